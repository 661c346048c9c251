/*
 * mi355zk.h -- C ABI of libmi355zk.so: the MI355X (gfx950) backend for the BN254 MSM / Fr-NTT hot
 * path of kobigurk/phase2-bn254.
 *
 * The reference has no FFI seam; the two Rust functions a maintainer would redirect are
 *   bellman/src/multiexp.rs:330-355   pub fn multiexp(pool, bases, density_map, exponents)
 *   bellman/src/domain.rs:263-272     fn best_fft(a, worker, omega, log_n)
 *   (+ the O(m) scalings of EvaluationDomain::{ifft, coset_fft, icoset_fft}, domain.rs:159-203)
 * INTEGRATION.md shows the Rust `extern "C"` block and the two call-site patches.
 *
 * Conventions (all integers little endian):
 *   Fq / Fr element   = 32 bytes = u64[4], least-significant limb first, MONTGOMERY form x*2^256 mod p,
 *                       fully reduced: the in-memory form of the reference's `Fq`/`Fr`, i.e. what
 *                       `into_raw_repr()` exposes (pairing/src/bn256/ec.rs:659-660).
 *   FrRepr (scalar)   = 32 bytes = u64[4], CANONICAL integer < r: the output of `into_repr()`
 *                       (the element type of multiexp's `exponents`, multiexp.rs:334).
 *   G1 affine base    = 64 bytes  x || y            (RawEncodable layout, ec.rs:653-664)
 *   G2 affine base    = 128 bytes x.c0 || x.c1 || y.c0 || y.c1
 *                       the ALL-ZERO record is the point at infinity (ec.rs:673-675).  The caller's own
 *                       records -- `G1Affine { x, y, infinity: bool }`, 72 B; G2Affine, 136 B (ec.rs:14-18),
 *                       whose identity is x = 0, y = R, infinity = true -- go to the STRIDED entry points
 *                       (mi355zk_bn254_g{1,2}_msm_strided, mi355zk_bases_cache_pin_strided) as they lie in
 *                       memory: the library repacks them on the device.  That is the path the Rust shim takes.
 *   Jacobian result   = X || Y || Z (12 / 24 u64), Z == 0 <=> infinity (ec.rs:227-246).  Any
 *                       representative of the group element may be returned (projective equality is
 *                       by value, ec.rs:45-85).
 *   density           = NULL for FullDensity (source.rs:80-99); else bit i of the map is
 *                       (density[i/32] >> (i%32)) & 1, `density_bits` bits long (DensityTracker,
 *                       source.rs:101-118).  Bases are COMPACTED: only set bits consume a base.
 *
 * Return codes:
 *   0  ok
 *   1  UnexpectedIdentity: a selected base with a non-zero exponent is infinity   (source.rs:50-52)
 *   2  UnexpectedEof:      the bases ran out                                      (source.rs:46-48,62-64)
 *   3  bad arguments (NULL pointer, log_n > 28 = PolynomialDegreeTooLarge domain.rs:66-79, sizes >= 2^31, an exponent
 *      >= 2^254, i.e. not a canonical FrRepr: mi355zk_last_error_index() names it)
 *  4 .. 8  the GroupDecodingError of a wire record (the point codecs and the accumulator entry points below), 5 = NotInSubgroup
 *  9  PointAtInfinity: a record of an accumulator file is the point at infinity (the accumulator entry points)
 *  <0  device failure (details on stderr).  There is NO CPU fallback inside the library.
 * When both error kinds are present the one at the lowest exponent index is reported (the reference's
 * answer depends on thread scheduling there; see oracle/tmpl_multiexp.h).
 *
 * Threading: every entry point may be called concurrently from several host threads (the prover
 * queues 8 multiexps before waiting, bellman/src/groth16/prover.rs:250-298); calls on one device are
 * serialised internally.  Entry points are synchronous: the result is complete on return, which a
 * futures-0.1 shim wraps in `future::result` (what singlecore::Worker::compute does, singlecore.rs:33-47).
 */
#ifndef MI355ZK_H
#define MI355ZK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355ZK_OK 0
#define MI355ZK_ERR_UNEXPECTED_IDENTITY 1
#define MI355ZK_ERR_UNEXPECTED_EOF 2
#define MI355ZK_ERR_BAD_ARGS 3
#define MI355ZK_ERR_POINT_AT_INFINITY 9 /* 4 .. 8 are the GroupDecodingError kinds of the point codecs */
#define MI355ZK_ERR_DEVICE (-1)

/* EvaluationDomain operations (domain.rs:154-203) for mi355zk_bn254_fr_domain_op[_dev] */
#define MI355ZK_OP_FFT 0
#define MI355ZK_OP_IFFT 1
#define MI355ZK_OP_COSET_FFT 2
#define MI355ZK_OP_ICOSET_FFT 3

/* ---- lifecycle.  device_ids == NULL / n_devices == 0: use the process's current HIP device.  The LAST call defines the
 * library's device set.
 *   n_devices == 1: one GPU (device_ids[0] is selected with hipSetDevice) -- one rank per GPU under torch.distributed / RCCL
 *                   (shard.py), or a single-GPU process.
 *   n_devices  > 1: SINGLE-PROCESS MULTI-GPU MODE, for the consumer this library is a drop-in for: one Rust process
 *                   (phase2/src/bin/prove.rs -> bellman/src/groth16/prover.rs:250-298 -> multiexp.rs:330-355) driving the 8 GPUs of a
 *                   node.  mi355zk_bn254_g{1,2}_msm (host buffers) with >= 2^20 exponents (env MI355ZK_MULTI_MIN_LOG) is then cut
 *                   into one cell per device -- contiguous point ranges, each evaluated by the single-GPU pipeline on its
 *                   own device from its own host thread, its exponents streamed over that device's PCIe link, its copy of a PINNED
 *                   base vector kept resident there -- and the n_devices Jacobian partials are joined on the host ("D2H of 8
 *                   records": no collective inside one process).  Result, return code and mi355zk_last_error_index are those of
 *                   the single-device call (the error at the lowest exponent index wins).  Shorter calls run whole, on the devices
 *                   of the set in turn, so a prover's eight concurrent multiexps spread over the node.  The calling thread's
 *                   current device is device_ids[0] on return and is left alone by the multiexps.  Device-pointer (`_dev`) entry
 *                   points are unaffected: their buffers live on one device, the caller's current one.  An id may be repeated
 *                   (logical devices sharing a GPU): that is how the mode is tested on a one-GPU box.
 * Returns 3 for an id that is not a visible device, < 0 if a device is not gfx950.  Replaces nothing in the reference (it has no
 * device). */
int mi355zk_init(const int *device_ids, int n_devices);
/* number of (logical) devices host-buffer multiexps are spread over: 1 unless mi355zk_init was given more */
int mi355zk_device_count(void);
/* GPUs visible to the process (hipGetDeviceCount; 0 when there is none or no driver): the ids 0 .. count-1 are what a caller
 * without HIP bindings of its own passes to mi355zk_init */
int mi355zk_visible_devices(void);
void mi355zk_shutdown(void);
const char *mi355zk_version(void);
/* The ABI revision this library was built with; a binding compares it with the MI355ZK_ABI_VERSION of the header it was written against
 * and refuses to run on a mismatch (lib.py and integration/mi355zk.rs do).  Bumped whenever a prototype or the meaning of an argument
 * changes: 6 = round 5's breaks -- batch_exp's `same_scalar` and point_fft's `inverse` became the bit masks `mode` (a legacy "true" of 2
 * would now read as MI355ZK_G2_TRUSTED_SUBGROUP), sparse_matvec[_dev] gained a trailing `flags`; 7 = the strided record entry points
 * (mi355zk_bn254_g{1,2}_msm_strided, mi355zk_bases_cache_pin_strided, mi355zk_bn254_g{1,2}_records_pack_dev). */
#define MI355ZK_ABI_VERSION 7
int mi355zk_abi_version(void);

/* ---- multiexp: host buffers.  Replaces bellman/src/multiexp.rs:330 `multiexp` for
 * S = (Arc<Vec<G1Affine>>, usize) (source.rs:36-70); `base_offset` is that usize. */
int mi355zk_bn254_g1_msm(const uint8_t *bases, size_t n_bases, size_t base_offset,
                         const uint64_t *scalars, size_t n_scalars,
                         const uint32_t *density, size_t density_bits,
                         uint64_t out_xyz[12]);
/* The CRS is an immutable `Arc<Vec<G>>` reused by every proof (groth16/mod.rs:216-238).  A caller that can PROMISE that --
 * the Rust shim keeps a clone of the Arc in a registry, so the allocation is neither rewritten nor freed, and pins the `Vec<G>` itself
 * with mi355zk_bases_cache_pin_strided (below) -- pins the vector: mi355zk_bases_cache_pin(ptr, n_bases, group 1|2).  Host-buffer calls over exactly (ptr, n_bases) then keep
 * their uploaded copy on the device and only the scalars cross PCIe after the first call (large calls are streamed: chunked
 * upload overlapped with the kernels).  Vectors that were NOT pinned are uploaded on every call: the plain `const uint8_t*`
 * entry is correct whatever the caller does with its buffer between calls.  mi355zk_bases_cache_invalidate(ptr) ends the
 * promise and drops the device copy (NULL: every vector) -- call it before rewriting or freeing a pinned vector.  A
 * fingerprint of sampled records is re-checked on every call as a second line of defence.  LRU-bounded by env
 * MI355ZK_BASES_CACHE_GB (default 64, 0 = off); env MI355ZK_BASES_CACHE_IMPLICIT=1 treats every vector as pinned. */
int mi355zk_bases_cache_pin(const void *host_bases, size_t n_bases, int group);
/* the same promise, and the library may also keep the vector's WINDOW TABLE on the device (table mode, below: n_windows times the
 * vector, inside MI355ZK_BASES_CACHE_GB): host-buffer calls over it that are not cut into chunks (< 2^23 exponents) then run in
 * table mode from the second call on -- what a prover wants for the h / l / a / b vectors of its Parameters. */
int mi355zk_bases_cache_pin_tables(const void *host_bases, size_t n_bases, int group);
void mi355zk_bases_cache_invalidate(const void *host_bases);
/* diagnostics: 1 when device copies of (parts of) the vector at host_bases are cached, else 0; *device_bytes = their total over all devices -- the whole
 * vector on the one device that runs the calls over it, or, after multi-GPU calls (mi355zk_init with n_devices > 1), one slice per device: n / N
 * records each -- and *table_bytes = the size of its window table or 0 */
int mi355zk_bases_cache_info(const void *host_bases, size_t *device_bytes, size_t *table_bytes);
/* Same for G = G2Affine (prover.rs:297-298). */
int mi355zk_bn254_g2_msm(const uint8_t *bases, size_t n_bases, size_t base_offset,
                         const uint64_t *scalars, size_t n_scalars,
                         const uint32_t *density, size_t density_bits,
                         uint64_t out_xyz[24]);

/* ---- multiexp over the CALLER's record layout (strided records).  bellman keeps its CRS as `Arc<Vec<G1Affine>>` of
 * `{ x: Fq, y: Fq, infinity: bool }` records (72 B; G2Affine 136 B, ec.rs:14-18) with the coordinates already in this ABI's form
 * (Montgomery u64[4] little endian; G2: c0 || c1).  These entry points take such a vector as it lies in memory: record i starts at
 * bases + i * stride; x is the 32 (G1) / 64 (G2) bytes at x_off, y those at y_off; when inf_off != MI355ZK_NO_FLAG and the byte at
 * inf_off is non-zero the record is the identity whatever its coordinates hold, otherwise the coordinates are taken as they are
 * (all-zero is still the identity).  The raw records cross PCIe in bounded pieces and are repacked on the device by the records_pack
 * kernel (no host-side conversion, no host copy); the MSM kernels are those of the packed entry points.  Result, return codes and
 * mi355zk_last_error_index are exactly those of mi355zk_bn254_g{1,2}_msm on the packed vector -- UnexpectedIdentity for a flagged base
 * under a non-zero exponent, UnexpectedEof, the multi-device cells of mi355zk_init's device set.
 * Returns 3 before any device work when: stride is 0, not a multiple of 4 or > 4096; x_off or y_off is not a multiple of 4; a
 * coordinate runs past stride; the x and y ranges overlap; inf_off (unless MI355ZK_NO_FLAG) is >= stride or inside a coordinate; or for
 * the limits of the packed form (NULL pointers, sizes >= 2^31).  stride 64 / 128, x_off 0, y_off 32 / 64, no flag IS the packed layout and
 * takes the packed path unchanged. */
#define MI355ZK_NO_FLAG ((size_t)-1)
int mi355zk_bn254_g1_msm_strided(const void *bases, size_t n_bases, size_t stride, size_t x_off, size_t y_off, size_t inf_off,
                                 size_t base_offset, const uint64_t *scalars, size_t n_scalars,
                                 const uint32_t *density, size_t density_bits, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_msm_strided(const void *bases, size_t n_bases, size_t stride, size_t x_off, size_t y_off, size_t inf_off,
                                 size_t base_offset, const uint64_t *scalars, size_t n_scalars,
                                 const uint32_t *density, size_t density_bits, uint64_t out_xyz[24]);
/* mi355zk_bases_cache_pin for a strided vector (same promise: the records are neither rewritten nor freed until
 * mi355zk_bases_cache_invalidate(host_bases)).  The layout is part of the pin and of the cache entry: a vector pinned under one layout
 * is served to strided calls with that layout only, and the same pointer pinned under two layouts is two entries.  The device copy
 * is the PACKED vector (mi355zk_bases_cache_info reports n * 64 / n * 128 bytes).  flags: MI355ZK_PIN_TABLES also keeps the window
 * table (as mi355zk_bases_cache_pin_tables).  mi355zk_bases_cache_invalidate(host_bases) drops every layout pinned there.  Returns 3
 * for a bad layout (the rules above), a bad group, NULL / n_bases == 0, or unknown flag bits. */
#define MI355ZK_PIN_TABLES 1u
int mi355zk_bases_cache_pin_strided(const void *host_bases, size_t n_bases, size_t stride, size_t x_off, size_t y_off,
                                    size_t inf_off, int group, uint32_t flags);
/* The repack kernel on device-resident records: n raw records at d_raw (layout as above) -> n packed records at d_out (64 / 128 B
 * each).  d_out must be 16-byte aligned and d_raw 4-byte aligned; the two may not overlap (3 otherwise).  Enqueued on `stream`
 * (a hipStream_t, NULL = the default stream); returns without waiting. */
int mi355zk_bn254_g1_records_pack_dev(const void *d_raw, size_t n, size_t stride, size_t x_off, size_t y_off, size_t inf_off,
                                      void *d_out, void *stream);
int mi355zk_bn254_g2_records_pack_dev(const void *d_raw, size_t n, size_t stride, size_t x_off, size_t y_off, size_t inf_off,
                                      void *d_out, void *stream);

/* ---- multiexp: bases and scalars already resident in HBM (the CRS / tau-table is reused across
 * calls: `Arc<Vec<G>>` inside groth16::Parameters, groth16/mod.rs:216-238).  `density` stays a HOST
 * pointer (it is tiny and the library needs its prefix sums).  `stream` is a hipStream_t (NULL = the
 * default stream); the call returns after the result has been copied back. */
int mi355zk_bn254_g1_msm_dev(const void *d_bases, size_t n_bases, size_t base_offset,
                             const void *d_scalars, size_t n_scalars,
                             const uint32_t *density, size_t density_bits,
                             void *stream, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_msm_dev(const void *d_bases, size_t n_bases, size_t base_offset,
                             const void *d_scalars, size_t n_scalars,
                             const uint32_t *density, size_t density_bits,
                             void *stream, uint64_t out_xyz[24]);
/* ---- verification multiexps of the ceremony code, device-resident inputs:
 * dense_multiexp (powersoftau/src/utils.rs:189-292): sum_i exp_i * base_i with bases.len() == exponents.len();
 * infinity bases add nothing and there are no Source errors.
 * merge_pairs (powersoftau/src/utils.rs:112-128; phase2/src/utils.rs:59-105; power_pairs = merge_pairs(v[0..n-1], v[1..])):
 * s = sum rho_i * v1_i and sx = sum rho_i * v2_i for ONE scalar vector rho -- digit extraction and sorts are
 * shared between the two sums.  rho are canonical FrRepr like every exponent of this ABI. */
int mi355zk_bn254_g1_dense_multiexp_dev(const void *d_bases, const void *d_scalars, size_t n, void *stream, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_dense_multiexp_dev(const void *d_bases, const void *d_scalars, size_t n, void *stream, uint64_t out_xyz[24]);
int mi355zk_bn254_g1_merge_pairs_dev(const void *d_v1, const void *d_v2, const void *d_rho, size_t n, void *stream, uint64_t out_s[12], uint64_t out_sx[12]);
int mi355zk_bn254_g2_merge_pairs_dev(const void *d_v1, const void *d_v2, const void *d_rho, size_t n, void *stream, uint64_t out_s[24], uint64_t out_sx[24]);
/* The same two on HOST buffers, over the device set of mi355zk_init (a single-process caller: powersoftau's verify_transform runs them over
 * 2^21 .. 2^28-point vectors): the sums are linear in the points, so the vectors are cut into pieces of 2^22 points, every piece is one
 * device call and the Jacobian partials are added on the host; the pieces are dealt to two host threads per device (one uploads while the
 * other computes).  Records and scalars as in the _dev forms; v1, v2 may overlap (power_pairs: v2 = v1 + one record).  Synchronous. */
int mi355zk_bn254_g1_dense_multiexp(const uint8_t *bases, const uint64_t *scalars, size_t n, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_dense_multiexp(const uint8_t *bases, const uint64_t *scalars, size_t n, uint64_t out_xyz[24]);
int mi355zk_bn254_g1_merge_pairs(const uint8_t *v1, const uint8_t *v2, const uint64_t *rho, size_t n, uint64_t out_s[12], uint64_t out_sx[12]);
int mi355zk_bn254_g2_merge_pairs(const uint8_t *v1, const uint8_t *v2, const uint64_t *rho, size_t n, uint64_t out_s[24], uint64_t out_sx[24]);
/* ---- the random exponents rho of merge_pairs, generated on the device.  The reference draws them from thread_rng (powersoftau/src/utils.rs:
 * 116-123, phase2/src/utils.rs:79-86); here they are a counter-based stream that a host can reproduce: ChaCha20 (constants "expand 32-byte k",
 * 20 rounds) with `key` in state words 4..11, a 64-bit block counter in words 12, 13 and `stream_id` in words 14, 15.  Scalar number g (a
 * 64-bit index) is words 8 (g & 1) .. 8 (g & 1) + 7 of block g >> 1: limb j = word[2 j] | word[2 j + 1] << 32, the top limb masked to 61
 * bits.  The value is uniform in [0, 2^253) and canonical without rejection (2^253 < r); a random linear combination over such scalars
 * accepts a false statement with probability 2^-253 per check.  The stream depends on (key, stream_id, g) alone -- not on the launch, not on
 * how a range is cut into calls or pieces.
 * fr_random_dev: scalars first .. first + n - 1 as canonical FrRepr (32 B each) at d_out (16-byte aligned); asynchronous on `stream`; n == 0
 * launches nothing; rc 3 on a NULL pointer, a misaligned d_out or n >= 2^31.  selftest_fr_random: the same values from the same code run on
 * the host (no device; out may be NULL when n == 0). */
int mi355zk_bn254_fr_random_dev(void *d_out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first, void *stream);
int mi355zk_selftest_fr_random(uint64_t *out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first);
/* merge_pairs with rho = scalars 0 .. n - 1 of the stream (key, stream_id): the _dev forms fill a stream-ordered workspace and run the
 * multiexp of merge_pairs_dev over it; the host-buffer forms upload no exponents -- every piece fills its own range of the stream on its
 * device -- so the two sums are the same points for every piece size and every device count.  A verifier takes `key` from the operating
 * system's generator and a distinct stream_id per vector. */
int mi355zk_bn254_g1_merge_pairs_random_dev(const void *d_v1, const void *d_v2, size_t n, const uint32_t key[8], uint64_t stream_id, void *stream, uint64_t out_s[12], uint64_t out_sx[12]);
int mi355zk_bn254_g2_merge_pairs_random_dev(const void *d_v1, const void *d_v2, size_t n, const uint32_t key[8], uint64_t stream_id, void *stream, uint64_t out_s[24], uint64_t out_sx[24]);
int mi355zk_bn254_g1_merge_pairs_random(const uint8_t *v1, const uint8_t *v2, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t out_s[12], uint64_t out_sx[12]);
int mi355zk_bn254_g2_merge_pairs_random(const uint8_t *v1, const uint8_t *v2, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t out_s[24], uint64_t out_sx[24]);
/* ONE WINDOW GROUP of a multiexp, for multi-GPU runs that shard by scalar windows as well as by point range: the windows of
 * the geometry chosen for n_scalars (a window count divisible by window_groups) are dealt out in window_groups equal groups
 * and only group `window_group` is evaluated: out = sum over its windows w of B^w * T_w.  The partials of all groups add up
 * (mi355zk_bn254_g{1,2}_add) to what mi355zk_bn254_g{1,2}_msm_dev returns; errors and their indices are those of the full
 * call.  (1, 0) is the full multiexp. */
int mi355zk_bn254_g1_msm_part_dev(const void *d_bases, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                  const uint32_t *density, size_t density_bits, uint32_t window_groups, uint32_t window_group,
                                  void *stream, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_msm_part_dev(const void *d_bases, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                  const uint32_t *density, size_t density_bits, uint32_t window_groups, uint32_t window_group,
                                  void *stream, uint64_t out_xyz[24]);
/* The general form: flags + window groups.  MI355ZK_MSM_SCALARS_MONTGOMERY: `d_scalars` holds Fr elements in MONTGOMERY form
 * (the prover's `Vec<Scalar<E>>` / `Vec<E::Fr>`) instead of canonical FrRepr -- the O(m) conversion passes
 * scalars_into_representations / field_elements_into_representations (bellman/src/groth16/prover.rs:89-129: `into_repr()` per
 * element) are fused into the digit extraction (one Montgomery reduction per scalar, no extra pass over HBM). */
#define MI355ZK_MSM_SCALARS_MONTGOMERY 1u
int mi355zk_bn254_g1_msm_ex_dev(const void *d_bases, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                const uint32_t *density, size_t density_bits, uint32_t flags, uint32_t window_groups, uint32_t window_group,
                                void *stream, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_msm_ex_dev(const void *d_bases, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                const uint32_t *density, size_t density_bits, uint32_t flags, uint32_t window_groups, uint32_t window_group,
                                void *stream, uint64_t out_xyz[24]);
/* ---- TABLE MODE: multiexps over a base vector that does not change between calls -- the `Arc<Vec<G>>` of groth16::Parameters
 * (bellman/src/groth16/mod.rs:216-238: every proof of a circuit queries the same h / l / a / b_g1 / b_g2) -- evaluated against a
 * precomputed WINDOW TABLE of that vector:  table[w * n_bases + i] = 2^(shift of window w) * bases[i]  for the n_windows windows of
 * mi355zk_msm_table_geometry(n_bases).  A digit of any window then belongs to the bucket of its value in ONE bucket set shared
 * by all windows: one reduction instead of one per window, and a wider window (fewer additions) on the 2^19 .. 2^24-point calls a
 * prover makes (nothing to gain at 2^26).  Same contract, result and errors as mi355zk_bn254_g{1,2}_msm_ex_dev
 * with window_groups = 1 (multiexp.rs:330-355; `base_offset` / `density` as there), at n_windows times the base memory.
 *   table_geometry:   window_bits / n_windows for a vector of n_bases points (group 1 = G1, 2 = G2): the table holds
 *                     n_windows * n_bases affine records (64 B / 128 B each).
 *   table_build_dev:  fills d_table (table_bytes >= n_windows * n_bases * record) from d_bases; d_table may start with the
 *                     bases themselves (d_table == d_bases: window 0 is the vector).  Synchronises `stream`.  One-time work.
 *                     Window w + 1 is window w doubled width[w] times (plain doublings, one batched normalisation): exact for
 *                     every point the decoders admit, in the order-r subgroup or not.
 *   msm_table_dev:    the multiexp; `n_bases` is the length of the ORIGINAL vector (the table's window stride). */
int mi355zk_msm_table_geometry(size_t n_bases, int group, uint32_t *window_bits, uint32_t *n_windows);
int mi355zk_bn254_g1_msm_table_build_dev(const void *d_bases, size_t n_bases, void *d_table, size_t table_bytes, void *stream);
int mi355zk_bn254_g2_msm_table_build_dev(const void *d_bases, size_t n_bases, void *d_table, size_t table_bytes, void *stream);
int mi355zk_bn254_g1_msm_table_dev(const void *d_table, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                   const uint32_t *density, size_t density_bits, uint32_t flags, void *stream, uint64_t out_xyz[12]);
int mi355zk_bn254_g2_msm_table_dev(const void *d_table, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                   const uint32_t *density, size_t density_bits, uint32_t flags, void *stream, uint64_t out_xyz[24]);
/* ---- BATCHED MULTIEXP: n_vectors exponent vectors against ONE base vector and ONE density map -- the shape of "many proofs over one
 * groth16::Parameters" (bellman/tests/mimc.rs:260-341 proves in a loop over one CRS; h / l / a / b_g1 / b_g2 and the density maps belong
 * to the circuit, the exponents to the witness).  Replaces a loop of n_vectors calls of mi355zk_bn254_g{1,2}_msm_ex_dev(..., flags, 1, 0,
 * ...): the vectors run as n_vectors x n_windows windows of one pipeline -- one launch sequence and one copy back -- which is what a
 * short multiexp (below ~2^18 exponents it does not fill the device) is made of.  Vector v is the n_scalars exponents at d_scalars +
 * v * scalar_stride * 32 bytes (`scalar_stride` in scalars, >= n_scalars; what lies between two vectors is not read); `base_offset`,
 * `density` and `flags` (MI355ZK_MSM_SCALARS_MONTGOMERY) as in msm_ex_dev, shared by all vectors.  out_xyz takes n_vectors Jacobian
 * points (12 / 24 words each).
 * ERRORS are per vector: rcs[v] and err_indices[v] are the return code and mi355zk_last_error_index() of the single call on vector v
 * (0 / -1: its point is in out_xyz; otherwise its words are untouched), whatever the other vectors hold: a pipeline pass that meets an
 * identity base under a non-zero exponent or a non-canonical exponent is discarded and its vectors are evaluated one by one, and so is
 * every vector when n_scalars reaches beyond the bases (UnexpectedEof).  Those are caller bugs; only the clean batch is fast.
 * The RETURN VALUE is 0 when the call ran (then rcs / err_indices are valid); 3 when it is refused as a whole, before any device work --
 * a NULL out_xyz / rcs / err_indices (or bases / scalars with a non-zero count), n_vectors == 0, scalar_stride < n_scalars, a size
 * >= 2^31, an unknown flag -- or the device code (-1).  n_vectors == 1 is msm_ex_dev(..., 1, 0, ...); n_scalars == 0 gives n_vectors
 * identities.  No window tables, window groups or host buffers here; a batch too large for one pass (4096 bucket sets, or the
 * workspace budget for long vectors) runs several passes inside the call.
 * msm_batch_geometry (diagnostic): the bucket sets one pass may hold, the windows of one vector of n_scalars exponents and the vectors
 * per pass the call above would take for (n_scalars, n_vectors); group 1 = G1, 2 = G2; any pointer may be NULL. */
int mi355zk_bn254_g1_msm_batch_dev(const void *d_bases, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                   size_t scalar_stride, size_t n_vectors, const uint32_t *density, size_t density_bits, uint32_t flags,
                                   void *stream, uint64_t *out_xyz /* n_vectors x 12 */, int *rcs, long long *err_indices);
int mi355zk_bn254_g2_msm_batch_dev(const void *d_bases, size_t n_bases, size_t base_offset, const void *d_scalars, size_t n_scalars,
                                   size_t scalar_stride, size_t n_vectors, const uint32_t *density, size_t density_bits, uint32_t flags,
                                   void *stream, uint64_t *out_xyz /* n_vectors x 24 */, int *rcs, long long *err_indices);
int mi355zk_msm_batch_geometry(size_t n_scalars, size_t n_vectors, int group, uint32_t *max_windows, uint32_t *n_windows, uint32_t *vectors_per_pass);
/* exponent index at which the last failing multiexp of this thread raised its error, or -1 */
long long mi355zk_last_error_index(void);
/* bits of the bucket field (c for the power-of-two window layouts, ceil(log2(B/2 + 1)) for the mixed-radix ones) and
 * the window count the library would use for n scalars (diagnostics / DESIGN.md section 4) */
int mi355zk_msm_window_bits(size_t n_scalars, int *n_windows);
/* the same for a run whose windows are dealt out in window_groups groups (the window count is then a multiple of it) */
int mi355zk_msm_window_bits_groups(size_t n_scalars, uint32_t window_groups, int *n_windows);

/* ---- Fr NTT.  Replaces bellman/src/domain.rs:263 `best_fft` for T = Scalar<Bn256>:
 * a[0..2^log_n) in place, natural order in and out, `omega` of order 2^log_n (Montgomery form).
 * Operand range, for every transform and domain entry point below: the elements of `a` (and omega and the scale factors) are CANONICAL
 * Montgomery Fr, stored words < r, unchecked.  That is the load state the kernels' lazy-reduction bounds are derived from
 * (csrc/ntt_butterfly.hpp; tests/cpp/test_ntt_bounds_host.cpp); the outputs are canonical again. */
int mi355zk_bn254_fr_ntt(uint64_t *a, uint32_t log_n, const uint64_t omega[4]);
/* EvaluationDomain::{fft, ifft, coset_fft, icoset_fft} (domain.rs:154-203) with the constants
 * `from_coeffs` derives for m = 2^log_n (domain.rs:84-98: omega, omegainv, geninv = 7^-1, minv). */
int mi355zk_bn254_fr_domain_op(uint64_t *a, uint32_t log_n, int op);
int mi355zk_bn254_fr_fft(uint64_t *a, uint32_t log_n);
int mi355zk_bn254_fr_ifft(uint64_t *a, uint32_t log_n);
int mi355zk_bn254_fr_coset_fft(uint64_t *a, uint32_t log_n);
int mi355zk_bn254_fr_icoset_fft(uint64_t *a, uint32_t log_n);
/* device-resident variants: asynchronous on `stream` (no host synchronisation). */
int mi355zk_bn254_fr_ntt_dev(void *d_a, uint32_t log_n, const uint64_t omega[4], void *stream);
/* (round 5) best_fft with the scalings around it fused in, for ANY factors -- distribute_powers(g) takes any g (domain.rs:176-189); the four
 * domain operations are this call with the domain's constants:
 *     a[i] *= pre_g^i   (if pre_g)        X[k] = sum_i a[i] * omega^(i k)        X[k] *= post_c * post_g^k   (each factor if given)
 * omega: a 2^log_n-th root of unity; all four are Montgomery forms (4 x u64); pre_g / post_c / post_g may be NULL.  Up to 2^20 the
 * factors live in a per-(omega, factors) copy of the inter-pass twiddle table (at most four per omega are kept; see DESIGN.md, NTT). */
int mi355zk_bn254_fr_ntt_scaled_dev(void *d_a, uint32_t log_n, const uint64_t omega[4], const uint64_t pre_g[4], const uint64_t post_c[4],
                                    const uint64_t post_g[4], void *stream);
int mi355zk_bn254_fr_domain_op_dev(void *d_a, uint32_t log_n, int op, void *stream);
/* (round 5) The same EvaluationDomain operation on `batch` (1 .. 64) DISTINCT device arrays of 2^log_n elements each, in place -- what
 * prover.rs:217-241 does to a, b and c one after the other (ifft, then coset_fft).  d_arrays: a HOST array of `batch` device pointers.
 * Results are those of `batch` calls of mi355zk_bn254_fr_domain_op_dev, byte for byte; every pass is ONE launch over the tiles of all
 * the arrays, so that one transform's loads and stores run under another's butterflies (2^20: 0.105 -> 0.087 ms per transform).
 * 3 = a null or repeated pointer, batch out of range, unknown op. */
int mi355zk_bn254_fr_domain_op_batch_dev(void *const *d_arrays, uint32_t batch, uint32_t log_n, int op, void *stream);
/* the domain constants themselves (Montgomery form), for callers that keep their own EvaluationDomain */
int mi355zk_bn254_fr_domain_constants(uint32_t log_n, uint64_t omega[4], uint64_t omegainv[4], uint64_t geninv[4], uint64_t minv[4]);

/* ---- elementwise Fr operations of EvaluationDomain on device-resident data (asynchronous on `stream`):
 * a[i] *= b[i] (mul_assign, domain.rs:236-249) and a[i] -= b[i] (sub_assign, domain.rs:251-260).
 * Operand range (these three entry points): every element is a Montgomery Fr as the reference holds one, i.e. a CANONICAL value < r on 4 x u64.
 * The kernels do not check it.  For an element >= r the call still returns 0 and the element's result is UNDEFINED (not even congruent to the
 * true product / difference in general: the product's reduction assumes a b < r 2^256, the difference one conditional correction); the results of
 * the other elements are unaffected.  A caller with unreduced data reduces it first. */
int mi355zk_bn254_fr_mul_assign_dev(void *d_a, const void *d_b, size_t n, void *stream);
int mi355zk_bn254_fr_sub_assign_dev(void *d_a, const void *d_b, size_t n, void *stream);
/* out[i] = into_repr(in[i]): Montgomery Fr -> canonical FrRepr (scalars_into_representations / field_elements_into_representations,
 * prover.rs:89-129) as a standalone pass; d_out may alias d_in.  (The multiexp can take Montgomery scalars directly: msm_ex_dev.) */
int mi355zk_bn254_fr_into_repr_dev(void *d_out, const void *d_in, size_t n, void *stream);
/* out[i] = in[i] * 2^256 mod r: canonical FrRepr -> Montgomery Fr (the inverse of mi355zk_bn254_fr_into_repr_dev); in < r, unchecked; may alias. */
int mi355zk_bn254_fr_from_repr_dev(void *d_out, const void *d_in, size_t n, void *stream);
/* ---- sparse matrix x vector over Fr (csrc/r1cs.hip): the evaluation of an R1CS on a witness, a[i] = sum_t coeff_t * w[var_t] over the terms
 * of constraint i (ProvingAssignment::enforce / eval, groth16/prover.rs:50-87), with the matrix resident on the device in CSR form.
 * out[r] = sum_{t = row_ptr[r]}^{row_ptr[r+1]-1} coeffs[coeff_id[t]] * x[col[t]],  r < n_rows   (all Montgomery Fr, canonical < r)
 * row_ptr: u32[n_rows + 1] from 0 to nnz, col: u32[nnz] (< n_x), coeff_id: u32[nnz] (< n_coeffs), coeffs: n_coeffs x 32 B, x: n_x x 32 B;
 * all device pointers; an empty row gives 0.  Asynchronous on `stream`, no host synchronisation.
 * The coefficients go through a table of DISTINCT values (a circuit has few: 1, -1, powers of two), 4 B per term instead of 32; a caller
 * without such a table passes coeff_id[t] = t.  Every term is multiplied (the reference skips the product by one: same field element), and
 * every step returns the canonical residue, so the result does not depend on the order of the summation.
 * Operand range: as for mul_assign / sub_assign above -- canonical Montgomery Fr, unchecked; an element >= r of x or coeffs makes the rows
 * that use it UNDEFINED, the call still returns 0 and the other rows are unaffected.
 * Index range: the call never reads or writes outside the arrays it was given, WHATEVER the index arrays hold -- every row's term range is
 * clamped to [0, nnz), and a term whose col >= n_x or coeff_id >= n_coeffs contributes nothing.  For such a structure the results are
 * unspecified, the call still returns 0 and nothing faults; it is not reported here, because that would cost a host synchronisation per
 * call: mi355zk_bn254_fr_sparse_matvec_check_dev below validates a matrix ONCE, synchronously.
 * 3 (before any device work) = a NULL pointer with a non-zero count; n_rows, nnz, n_x or n_coeffs >= 2^32; d_out == d_x.
 * n_rows == 0 succeeds and launches nothing. */
int mi355zk_bn254_fr_sparse_matvec_dev(void *d_out, const uint32_t *d_row_ptr, const uint32_t *d_col, const uint32_t *d_coeff_id,
                                       const void *d_coeffs, size_t n_coeffs, const void *d_x, size_t n_x, size_t n_rows, size_t nnz, void *stream);
/* Synchronous structural check, once per matrix: 0, or 3 if row_ptr is not monotone from 0 to nnz, a col >= n_x or a coeff_id >= n_coeffs
 * (and for the argument errors of the evaluating call, before any device work). */
int mi355zk_bn254_fr_sparse_matvec_check_dev(const uint32_t *d_row_ptr, const uint32_t *d_col, const uint32_t *d_coeff_id,
                                             size_t n_coeffs, size_t n_x, size_t n_rows, size_t nnz, void *stream);
/* ---- a batch of witnesses over one circuit (csrc/r1cs.hip): the same matrix times n_vectors vectors in ONE launch, and the satisfaction
 * check of the result.  No more than MI355ZK_R1CS_MAX_VECTORS vectors per call (the second grid dimension of both kernels). */
#define MI355ZK_R1CS_MAX_VECTORS 65535
/* sparse_matvec_dev for n_vectors vectors: vector v is the n_x elements at d_x + v * x_stride * 32 bytes, its result the n_rows elements
 * at d_out + v * out_stride * 32 bytes (strides in elements, as scalar_stride in msm_batch_dev; what lies between two vectors is neither
 * read nor written).  A term's col, coeff_id and coefficient are loaded once per tile of vectors; every step returns the canonical residue,
 * so out[v] is byte for byte what the single call writes for x[v], and n_vectors == 1 is the single call.  Operand and index range as
 * above.  Asynchronous on `stream`, no host synchronisation.
 * 3 (before any device work) = what the single call refuses; n_vectors == 0 or > MI355ZK_R1CS_MAX_VECTORS; x_stride < n_x; out_stride <
 * n_rows; an out range [d_out, d_out + ((n_vectors - 1) out_stride + n_rows) 32) that overlaps the x range.  n_rows == 0 succeeds and
 * launches nothing. */
int mi355zk_bn254_fr_sparse_matvec_batch_dev(void *d_out, size_t out_stride, const uint32_t *d_row_ptr, const uint32_t *d_col,
                                             const uint32_t *d_coeff_id, const void *d_coeffs, size_t n_coeffs, const void *d_x, size_t n_x,
                                             size_t x_stride, size_t n_vectors, size_t n_rows, size_t nnz, void *stream);
/* Is the R1CS satisfied: a[i] * b[i] == c[i] for every row i < n_rows of every vector (SynthesisError::Unsatisfiable, bellman/src/cs.rs:162;
 * the reference's Groth16 path has no such check and leaves a wrong witness to the pairing).  d_a, d_b, d_c are device arrays of Montgomery
 * Fr, read only; vector v's rows start at base + v * vector_stride * 32 bytes (stride in elements, >= n_rows); the three may be slices of
 * one array -- the layout of the product above: a = out, b = out + m, c = out + 2 m, vector_stride >= 3 m.  first_bad[v] (HOST, n_vectors
 * entries) is the lowest failing row of vector v or -1, n_bad[v] (HOST, may be NULL) the number of failing rows.  Synchronises `stream`.
 * Operand range: canonical Montgomery Fr, which is what the product writes; for other words the verdict is unspecified, nothing faults.
 * 3 (before any device work) = a NULL array with n_rows > 0; a NULL first_bad; n_vectors == 0 or > MI355ZK_R1CS_MAX_VECTORS;
 * vector_stride < n_rows; n_rows >= 2^32.  n_rows == 0 fills -1 / 0 without device work.
 * mi355zk_selftest_r1cs_check: the same row predicate on three HOST arrays of n_rows x 4 u64 (one vector, no device). */
int mi355zk_bn254_fr_r1cs_check_dev(const void *d_a, const void *d_b, const void *d_c, size_t n_rows, size_t vector_stride, size_t n_vectors,
                                    long long *first_bad, uint32_t *n_bad, void *stream);
int mi355zk_selftest_r1cs_check(const uint64_t *a, const uint64_t *b, const uint64_t *c, size_t n_rows, long long *first_bad, uint32_t *n_bad);
/* EvaluationDomain::divide_by_z_on_coset (domain.rs:207-234): a[i] *= (g^m - 1)^-1 with m = 2^log_n and g = 7 the multiplicative
 * generator (z(tau) = tau^m - 1, domain.rs:207-212) -- the division step of the prover's H polynomial (prover.rs:217-241), so that
 * the whole ifft / coset_fft / mul / sub / divide / icoset_fft pipeline stays in HBM.  Asynchronous on `stream`. */
int mi355zk_bn254_fr_divide_by_z_on_coset_dev(void *d_a, uint32_t log_n, void *stream);
/* The three elementwise steps of the H polynomial in ONE pass: a[i] = (a[i] * b[i] - c[i]) * zinv with zinv = (7^(2^log_n) - 1)^-1, i.e.
 * mul_assign(a, b), sub_assign(a, c), divide_by_z_on_coset(a) (prover.rs:232-236), byte for byte, at three loads and one store per element
 * instead of five loads and three stores.  n may be any length; log_n (<= 28) only selects z.  Operand range as for mul_assign / sub_assign
 * above (canonical Montgomery Fr, unchecked).  d_a may not alias d_b or d_c.  Asynchronous on `stream`.  3 = a NULL pointer with n > 0, log_n > 28. */
int mi355zk_bn254_fr_h_combine_dev(void *d_a, const void *d_b, const void *d_c, size_t n, uint32_t log_n, void *stream);
/* The prover's H evaluation (prover.rs:216-248) on three DISTINCT device arrays of 2^log_n Montgomery Fr each: ifft and coset_fft of a, b, c
 * (two mi355zk_bn254_fr_domain_op_batch_dev calls over the three), h_combine, icoset_fft of a and, with MI355ZK_H_INTO_REPR in
 * `flags`, into_repr of every element.  On return (asynchronous on `stream`, no host synchronisation) d_a[0 .. 2^log_n) is what icoset_fft
 * leaves -- the caller uses the first 2^log_n - 1 elements (prover.rs:243-246 drops the last coefficient) -- and d_b, d_c are SCRATCH: their
 * contents are unspecified.  Byte-identical to the ten calls it replaces.  3 = a NULL or repeated pointer, log_n > 28, unknown flag bits. */
#define MI355ZK_H_INTO_REPR 1u
int mi355zk_bn254_fr_h_poly_dev(void *d_a, void *d_b, void *d_c, uint32_t log_n, uint32_t flags, void *stream);
/* The same chain on HOST buffers, for a caller that holds `Vec<Scalar>`s (every Rust or C caller): a, b, c each hold `len` <= 2^log_n
 * Montgomery Fr and are zero-padded to 2^log_n on the device, as EvaluationDomain::from_coeffs does (domain.rs:66-98); h receives the first
 * 2^log_n - 1 elements of the result (none for log_n == 0, and the call still succeeds), canonical FrRepr with MI355ZK_H_INTO_REPR, else
 * Montgomery.  128 B per element cross the link instead of the 448 B of seven mi355zk_bn254_fr_domain_op calls, the uploads in bounded
 * pinned pieces that overlap the transforms of the array before.  Runs on the calling thread's current device; re-entrant from several host
 * threads; device buffers and streams are leased from the library's pools.  a, b, c are never written.  Synchronous.
 * 3 (before any device work) = a NULL pointer, log_n > 28, len == 0 or len > 2^log_n, unknown flag bits, h equal to a, b or c.
 * On ANY non-zero return the contents of h are unspecified and a, b, c are intact: the caller can fall back to its CPU path. */
int mi355zk_bn254_fr_h_poly(uint64_t *h, const uint64_t *a, const uint64_t *b, const uint64_t *c, size_t len, uint32_t log_n, uint32_t flags);
/* EvaluationDomain::z (domain.rs:207-212): out = tau^(2^log_n) - 1, Montgomery in and out (host arithmetic). */
int mi355zk_bn254_fr_domain_z(uint32_t log_n, const uint64_t tau[4], uint64_t out[4]);
/* out[i] = coeff * base^i for i < n, Montgomery in and out (device array of n x 32 B; base and coeff by value from the host): the powers of
 * tau of groth16/generator.rs:256-269 (per-chunk `pow` and a running product there) and, with coeff = z(tau) / delta, the H-query exponents
 * of :288-296.  The host squares base 31 times; every lane owns 16 consecutive indices, forms coeff * base^(16 lane) from the set bits of
 * its index (at most 28 products) and walks its run with one product per element.  Operand range as for mul_assign above.  Asynchronous
 * on `stream`.  n == 0 succeeds and launches nothing.  3 = a NULL pointer with n > 0, n >= 2^32. */
int mi355zk_bn254_fr_powers_dev(void *d_out, const uint64_t base[4], const uint64_t coeff[4], size_t n, void *stream);
/* ---- a polynomial against points (csrc/fr_poly.hip): evaluation at z and division by (x - z) on device-resident coefficients, the two Fr
 * steps of a KZG opening -- kate_divison (bellman/src/sonic/util.rs:444-463: q[n-2] = a[n-1], q[i-1] = a[i] + z q[i], serial there) and
 * evaluate_at_consequitive_powers (sonic/util.rs:151-200, with first_power = 1).  coeffs: n x 32 B on the device, lowest degree first; z: n_points
 * x 4 u64 on the HOST, read before the call returns; everything Montgomery Fr.  The recurrence is a suffix scan and runs as three launches (run and
 * tile aggregates, tile carries, apply; evaluation is the first two) for all the points at once, the point being the second grid dimension, hence
 * MI355ZK_POLY_MAX_POINTS.  Every step returns the canonical residue, so the results are the serial recurrence's byte for byte.
 * Operand range: as for mul_assign / sub_assign above -- canonical Montgomery Fr, unchecked; a coefficient >= r makes the quotient elements below
 * it and the remainder UNDEFINED, a point >= r everything of that point; the call still returns 0 and nothing faults.
 * Both calls are asynchronous on `stream` (no host synchronisation); their scratch is the library's, per (device, stream).
 * eval:   out[j] = sum_i coeffs[i] z_j^i; n == 0 gives 0.
 * divide: coeffs(x) = q_j(x) (x - z_j) + rem_j, q_j = the n - 1 elements at d_q + j * q_stride * 32 B (stride in elements; what lies between two
 *         quotients is neither read nor written), rem_j = coeffs(z_j) at d_rem + j * 32 B unless d_rem is NULL.  n == 1 writes no quotient and
 *         rem = coeffs[0]; n == 0 writes no quotient and rem = 0.  d_q may not overlap d_coeffs.
 * 3 (before any device work) = a NULL pointer with a non-zero count (d_rem apart); n >= 2^32; n_points == 0 or > MI355ZK_POLY_MAX_POINTS;
 * q_stride < n - 1; a quotient range [d_q, d_q + ((n_points - 1) q_stride + n - 1) 32) that overlaps the coefficients. */
#define MI355ZK_POLY_MAX_POINTS 65535
int mi355zk_bn254_fr_poly_eval_dev(void *d_out, const void *d_coeffs, size_t n, const uint64_t *z, size_t n_points, void *stream);
int mi355zk_bn254_fr_poly_divide_dev(void *d_q, size_t q_stride, void *d_rem, const void *d_coeffs, size_t n, const uint64_t *z, size_t n_points,
                                     void *stream);
/* The same routines compiled for the host, in the kernels' grouping into runs, tiles and carry chunks: one point, no device.  q: n - 1 elements
 * (may be NULL for n <= 1), rem = coeffs(z).  3 = a NULL pointer with a non-zero count, n >= 2^32. */
int mi355zk_selftest_fr_poly_divide(uint64_t *q, uint64_t rem[4], const uint64_t *coeffs, size_t n, const uint64_t z[4]);
/* The compile-time geometry: coefficients per lane, coefficients per workgroup (tile), tiles per chunk of the carry kernel -- the sizes at
 * which the code takes another path, for tests. */
int mi355zk_fr_poly_geometry(uint32_t *run, uint32_t *tile, uint32_t *carry_width);
/* ---- batch inversion (csrc/fr_inverse.hip): Montgomery's trick over runs, tiles and a product tree per tile; three launches and ONE Fermat
 * inversion per call.
 * out[i] = in[i]^-1 (Montgomery Fr in and out, canonical < r, unchecked as for mul_assign); in[i] == 0 gives out[i] = 0.
 * d_out may be d_in exactly (in place); any other overlap is refused.  d_n_zero: NULL, or a DEVICE uint32 that receives the number of zero
 * elements.  Asynchronous on `stream`, no host synchronisation; scratch is the library's, per (device, stream).
 * n == 0 succeeds and launches nothing (and still clears *d_n_zero).  3 = NULL array with n > 0, n >= 2^32, partial overlap. */
int mi355zk_bn254_fr_batch_inverse_dev(void *d_out, const void *d_in, size_t n, uint32_t *d_n_zero, void *stream);
/* The same lane routines compiled for the host, in the kernels' grouping into runs, tiles and carry chunks: no device.  out may be in;
 * n_zero may be NULL.  3 = a NULL array with n > 0, n >= 2^32. */
int mi355zk_selftest_fr_batch_inverse(uint64_t *out, const uint64_t *in, size_t n, uint32_t *n_zero);
/* The compile-time geometry: elements per lane, elements per workgroup (tile), tile products per chunk of the second launch. */
int mi355zk_fr_inverse_geometry(uint32_t *run, uint32_t *tile, uint32_t *carry_width);
/* ---- prefix scans (csrc/fr_scan.hip): running products c_i = a_i c_{i-1} (GrandProductArgument::new, bellman/src/sonic/unhelped/
 * grand_product_argument.rs:94-172, serial there) and running sums of device-resident rows, over runs, tiles and carry chunks in three launches
 * (run and tile aggregates; one workgroup per row scans the tile aggregates; apply).  Rows of one tile take the third launch alone.
 * `rows` vectors of n Montgomery Fr: row r is the n elements at base + r * stride * 32 B (strides in elements; what lies between two rows is
 * neither read nor written).  n outputs per row in either mode:
 *   inclusive (default)         out[i] = in[0] o .. o in[i]
 *   MI355ZK_SCAN_EXCLUSIVE      out[0] = the identity (Montgomery one / zero), out[i] = in[0] o .. o in[i-1]
 * d_total: NULL, or rows x 32 B on the device: every row's aggregate over all n elements (the identity for n == 0).
 * A zero is an ORDINARY element of a product: everything after it in its row is zero, exactly as in the serial chain.  This is NOT the
 * convention of batch_inverse_dev above, which skips zeros.  Every step returns the canonical residue, so the outputs are the serial chain's
 * byte for byte.  Operand range as for mul_assign (canonical Montgomery Fr, unchecked; an element >= r makes its row UNDEFINED from there on).
 * d_out == d_in with equal strides is allowed (in place); any other overlap of the two ranges [base, base + ((rows - 1) stride + n) 32), or
 * of d_total with either, is refused.  Asynchronous on `stream`, no host synchronisation; scratch is the library's, per (device, stream).
 * n == 0 or rows == 0 launches nothing except what fills d_total.
 * 3 (before any device work) = a NULL array with non-zero work; n >= 2^32; rows > 65535; a stride < n with rows > 1; unknown flag bits;
 * partial overlap. */
#define MI355ZK_SCAN_SUM        1u   /* running sums; default: running products */
#define MI355ZK_SCAN_EXCLUSIVE  2u   /* out[0] = identity, out[i] = in[0] o .. o in[i-1]; default inclusive: out[i] = in[0] o .. o in[i] */
int mi355zk_bn254_fr_scan_dev(void *d_out, size_t out_stride, const void *d_in, size_t in_stride, size_t n, size_t rows,
                              uint32_t flags, void *d_total, void *stream);
/* The scan of term[i] = num[i] * den[i]^-1: the grand product Z[i+1] = Z[i] num[i] / den[i] of a permutation argument (exclusive product), the
 * log-derivative sum S[i+1] = S[i] + num[i] / den[i] (exclusive sum).  d_num == NULL: every num[i] is one.  The denominators are copied into
 * d_out (not when d_out == d_den exactly, with equal strides, which is allowed), inverted there by ONE batch inversion over all the rows -- one
 * Fermat inversion per call, however many rows -- and the scan runs in place over d_out with num multiplied in at load, so no array of terms
 * is formed.  den[i] == 0 gives den[i]^-1 = 0 by batch_inverse_dev's convention and the term 0; such elements are counted in *d_n_zero (a DEVICE
 * uint32, may be NULL; the call clears it first).  d_out may not overlap d_num, nor d_den except as above.  Otherwise as fr_scan_dev, the
 * refusals included. */
int mi355zk_bn254_fr_ratio_scan_dev(void *d_out, size_t out_stride, const void *d_num, size_t num_stride, const void *d_den, size_t den_stride,
                                    size_t n, size_t rows, uint32_t flags, void *d_total, uint32_t *d_n_zero, void *stream);
/* a[i] += c * b[i] (mul_add_polynomials, bellman/src/sonic/util.rs:855-873); d_b == NULL: a[i] += c, the reference's all-ones vector without the
 * vector.  c: Montgomery, on the HOST, read before the call returns.  Operand range as for mul_assign.  Asynchronous on `stream`.
 * 3 = a NULL d_a with n > 0, a NULL c. */
int mi355zk_bn254_fr_mul_add_dev(void *d_a, const void *d_b, const uint64_t c[4], size_t n, void *stream);
/* The scan's lane routines compiled for the host, in the kernels' grouping into runs, tiles and carry chunks: one row, no device.  num may be
 * NULL, out may be in, total may be NULL.  3 = a NULL array with n > 0, n >= 2^32, unknown flag bits. */
int mi355zk_selftest_fr_scan(uint64_t *out, const uint64_t *in, const uint64_t *num, size_t n, uint32_t flags, uint64_t total[4]);
/* The compile-time geometry: elements per lane, elements per workgroup (tile), tile aggregates per chunk of the carry launch. */
int mi355zk_fr_scan_geometry(uint32_t *run, uint32_t *tile, uint32_t *carry_width);
/* ---- a polynomial in EVALUATION form against points (csrc/fr_evals.hip): the evaluation-form twin of fr_poly_divide_dev.
 * evals: 2^log_n Montgomery Fr on the device, evals[i] = p(omega^i) in natural order, omega = mi355zk_bn254_fr_domain_constants(log_n).
 * z: n_points x 4 u64 on the HOST (Montgomery), read before the call returns.  For every point j:
 *   values[j] = p(z_j)                                        at d_values + j * 32 B   (device; may not be NULL)
 *   q_j[i]    = ((p(x) - p(z_j)) / (x - z_j)) (omega^i)       2^log_n elements at d_q + j * q_stride * 32 B; d_q == NULL: values only
 * (q_stride in elements; what lies between two quotients is neither read nor written).  z_j may lie IN the domain (z_j = omega^k): then
 * values[j] = evals[k], and q_j[k] = -omega^-k * sum_{i != k} q_j[i] omega^i.  One batch inversion of the n_points 2^log_n denominators
 * omega^i - z_j, which are formed where the quotients go (in the library's scratch when d_q is NULL); the table of omega^i is scratch too.
 * Operand range as for mul_assign.  Asynchronous on `stream`.  3 = NULL evals / values / z, log_n > 28, n_points == 0 or >
 * MI355ZK_POLY_MAX_POINTS, and with a d_q: q_stride < 2^log_n, a quotient range that overlaps evals or values. */
int mi355zk_bn254_fr_evals_divide_dev(void *d_q, size_t q_stride, void *d_values, const void *d_evals, uint32_t log_n, const uint64_t *z,
                                      size_t n_points, void *stream);
/* Measured Montgomery-product rate of this library (the integer-ALU roofline the kernels are priced
 * against): `blocks` x 256 lanes each run 4 independent chains of `iters` products.  which: 0 Fq, 1 Fr.
 * out[0..3] = a*b^iters (Montgomery arithmetic, lane 0, chain 0) for a parity check; *ms = kernel time. */
int mi355zk_ubench_fp_mul(int which, uint32_t blocks, uint32_t iters, const uint64_t a[4], const uint64_t b[4], uint64_t out[16], float *ms);

/* ---- self-test hooks: the kernels' "U-form" arithmetic (29-bit lazy limbs, csrc/fieldu.hpp, curveu.hpp)
 * compiled for the HOST, so that it can be checked against the oracle / big-int model without a GPU. */
int mi355zk_selftest_u_mul(int which, const uint32_t a[9], const uint32_t b[9], uint32_t out[9]);
int mi355zk_selftest_u_mul_shoup(int which, const uint32_t a[9], const uint32_t w_plain[8], uint32_t out[9], uint32_t out_wq[9]);
int mi355zk_selftest_u_sub(int which, int k, int s, const uint32_t a[9], const uint32_t b[9], uint32_t out[9]);
int mi355zk_selftest_u_pack(int which, const uint64_t a_std[4], uint32_t out_u[9], const uint32_t in_u[9], uint64_t out_std[4]);
int mi355zk_selftest_u_reduce32(int which, const uint32_t in_u[9], uint64_t out_std[4]);
int mi355zk_selftest_g1_accumulate(int mode, const uint64_t *affine_pts, const uint8_t *negate, size_t n, uint64_t out_xyzz[16]);
int mi355zk_selftest_g1_record_sum(int mode, const uint64_t *affine_pts, const uint8_t *negate, const uint32_t *group, size_t n, size_t n_groups, uint64_t out_xyzz[16]);
int mi355zk_selftest_g2_record_sum(int mode, const uint64_t *affine_pts, const uint8_t *negate, const uint32_t *group, size_t n, size_t n_groups, uint64_t out_xyzz[32]);
/* The dense G1 multiexp over device buffers (as mi355zk_bn254_g1_dense_multiexp_dev; one chunk) that ALSO hands back what its accumulate stage left,
 * before the bucket reduction: first[b] / last[b], the bounds of bucket b's index list in vals (entries: base index, bit 31 = negate, in the order the
 * lane adds them), and the bucket array (records: 16 u64 per bucket -- X, Y, ZZ, ZZZ canonical, 2^261 domain; all zero: empty or infinity).
 * *n_buckets and *n_vals are always set; a capacity below them returns 3 with nothing copied. */
int mi355zk_selftest_g1_msm_buckets_dev(const void *d_bases, const void *d_scalars, size_t n, void *stream, uint64_t out_xyz[12], uint32_t *n_buckets,
                                        uint32_t *n_vals, uint32_t *first, uint32_t *last, size_t cap_buckets, uint32_t *vals, size_t cap_vals,
                                        uint64_t *records);
int mi355zk_selftest_msm_digits(size_t n_scalars, uint32_t window_groups, const uint32_t scalar[8], uint32_t w_start, uint32_t w_stop, int direct, int32_t *digits, uint32_t *geom);
int mi355zk_selftest_glv_split(const uint32_t k[8], uint32_t out[12]);
int mi355zk_selftest_glv_wnaf5(const uint32_t m[5], int8_t digits[164]);
int mi355zk_selftest_glv2_split(const uint32_t k[8], uint32_t out[10]);
int mi355zk_selftest_g2_psi(const uint64_t affine_pt[16], uint64_t out_xyz[24]);
int mi355zk_selftest_g2_scalar_mul_u(const uint64_t affine_pt[16], const uint64_t scalar[4], uint64_t out_xyz[24]);
int mi355zk_selftest_g2_accumulate(int mode, const uint64_t *affine_pts, const uint8_t *negate, size_t n, uint64_t out_xyzz[32]);
/* the fixed-base program of csrc/fixed_base.hpp on the host: the 32 signed 8-bit digits of k (sum digits[w] 2^(8 w) == k for k < r), and
 * k * base through the same recoding, step program and addition routine as the kernels, every table entry it needs computed by a plain host
 * scalar multiplication (group: 1 = G1, 8 + 8 u64; 2 = G2, 16 + 16 u64; 3 = a base the table build would refuse) */
int mi355zk_selftest_fixed_base_digits(const uint64_t k[4], int16_t digits[32]);
int mi355zk_selftest_fixed_base_mul(int group, const uint64_t *base_affine, const uint64_t k[4], uint64_t *out_affine);
/* one row of mi355zk_bn254_g1_fixed_bases_lincomb_dev on the host, the program of its one-slice lane: first + sum_j scalars[j] * bases[j]
 * (bases n_bases x 8 u64, scalars n_bases x 4 u64 canonical; first_affine may be NULL = the identity).  3 = a NULL pointer, a base off the curve */
int mi355zk_selftest_fixed_bases_lincomb(const uint64_t *bases_affine, size_t n_bases, const uint64_t *first_affine, const uint64_t *scalars,
                                         uint64_t out_affine[8]);

/* ---- self-test hook ON THE DEVICE: one primitive of csrc/field.hpp / fieldu.hpp / curveu.hpp per lane, on operands the caller chose, so
 * that the gfx950 object code -- and the code that exists in the device pass only: the Montgomery product of mont_mul_gfx950.inc, the quad-
 * and pair-per-bucket additions -- meets hand-made edge operands (tests/field_edge_vectors.py).  Host buffers: case i is in[i * in_words_per_case ..],
 * its result out[i * out_words_per_case ..]; the word counts are fixed per op (csrc/selftest_dev_ops.hpp: devop_shape) and a call with
 * others, an unknown op, `which` == 1 (Fr) for an Fq-only op, or n_cases == 0 / not a multiple of the op's lane group returns rc 3.  One case
 * per lane, 256 lanes per workgroup; the padding lanes repeat the last case.  The lane-group ops (_QUAD: 4 lanes, _PAIR_: 2) expect the SAME case
 * in every lane of a group and return every lane's result.  op | MI355ZK_DEVOP_CHAIN runs the build of the op with ZK_CHAIN_MAD (fieldu.hpp),
 * as msm_g1.hip and ntt.hip ship it: the U_ and G1_ ops only.  Field elements: 8 x 32-bit words (Fp), 9 x 29-bit limbs in u32 (U-form);
 * a register-form point is X, Y, ZZ, ZZZ in U-form, a record the same four coordinates as canonical Fp words. */
enum mi355zk_devop {
  MI355ZK_DEVOP_FP_MUL = 0, MI355ZK_DEVOP_FP_SQR, MI355ZK_DEVOP_FP_ADD, MI355ZK_DEVOP_FP_SUB, MI355ZK_DEVOP_FP_DBL, MI355ZK_DEVOP_FP_NEG, MI355ZK_DEVOP_FP_REDUCE_ONCE, MI355ZK_DEVOP_FP_INV,
  MI355ZK_DEVOP_FQ2_MUL, MI355ZK_DEVOP_FQ2_SQR, MI355ZK_DEVOP_FQ2_INV, MI355ZK_DEVOP_FQ2_ADD, MI355ZK_DEVOP_FQ2_SUB, MI355ZK_DEVOP_FQ2_NEG,
  MI355ZK_DEVOP_U_FROM_STD, MI355ZK_DEVOP_U_CARRY, MI355ZK_DEVOP_U_TO_STD_LT2P, MI355ZK_DEVOP_U_TO_STD_LT32P, MI355ZK_DEVOP_U_ADD, MI355ZK_DEVOP_U_DBL,
  MI355ZK_DEVOP_U_SUB_1_1, MI355ZK_DEVOP_U_SUB_2_1, MI355ZK_DEVOP_U_SUB_3_1, MI355ZK_DEVOP_U_SUB_4_1, MI355ZK_DEVOP_U_SUB_4_2, MI355ZK_DEVOP_U_SUB_4_3, MI355ZK_DEVOP_U_SUB_8_1, MI355ZK_DEVOP_U_SUB_16_1,
  MI355ZK_DEVOP_U_MUL, MI355ZK_DEVOP_U_SQR, MI355ZK_DEVOP_U_MUL2, MI355ZK_DEVOP_U_MUL3, MI355ZK_DEVOP_U_MUL4, MI355ZK_DEVOP_U_MUL_SHOUP, MI355ZK_DEVOP_U_IS_ZERO_LT2P, MI355ZK_DEVOP_U_IS_ZERO_LT8P,
  MI355ZK_DEVOP_F2U_MUL_2, MI355ZK_DEVOP_F2U_MUL_4, MI355ZK_DEVOP_F2U_MUL_8, MI355ZK_DEVOP_F2U_SQR_2, MI355ZK_DEVOP_F2U_SQR_4, MI355ZK_DEVOP_F2U_SQR_6, MI355ZK_DEVOP_F2U_SQR_8, MI355ZK_DEVOP_F2U_SUB_2, MI355ZK_DEVOP_F2U_SUB_3, MI355ZK_DEVOP_F2U_SUB_8,
  MI355ZK_DEVOP_G1_DOUBLE_AFFINE, MI355ZK_DEVOP_G1_DOUBLE, MI355ZK_DEVOP_G1_ADD_MIXED, MI355ZK_DEVOP_G1_RADD, MI355ZK_DEVOP_G1_RECORD_TRIP, MI355ZK_DEVOP_G1_RADD_QUAD, MI355ZK_DEVOP_G1_PAIR_ADD_MIXED,
  MI355ZK_DEVOP_G2_DOUBLE_AFFINE, MI355ZK_DEVOP_G2_DOUBLE, MI355ZK_DEVOP_G2_ADD_MIXED, MI355ZK_DEVOP_G2_RADD, MI355ZK_DEVOP_G2_RECORD_TRIP, MI355ZK_DEVOP_G2_RADD_QUAD, MI355ZK_DEVOP_G2_PAIR_ADD_MIXED,
  MI355ZK_DEVOP_G1_JAC_DOUBLE, MI355ZK_DEVOP_G1_JAC_ADD_MIXED, MI355ZK_DEVOP_G1_JAC_ADD_TAB,
  MI355ZK_DEVOP_G2_JAC_DOUBLE, MI355ZK_DEVOP_G2_JAC_ADD_TAB, MI355ZK_DEVOP_G2_JAC_TAB_PSI,
  MI355ZK_DEVOP_COUNT
};
/* Ops whose vectors live in a test file of their own (the enum above is, name by name, the table of tests/field_edge_vectors.py); the codes go on
 * from MI355ZK_DEVOP_COUNT.  G1_ADD_AFFINE_PAIR: xyzzu_from_affine_pair (curveu.hpp), how a bucket opens -- x1, y1, x2, y2 (Fp words), negate1,
 * negate2  ->  the accumulator (36 words), xyzzu_to_r of it (32); U-form over Fq, both builds.  tests/test_gpu_pair_start_op.py. */
enum mi355zk_devop_more {
  MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR = MI355ZK_DEVOP_COUNT,
  MI355ZK_DEVOP_END
};
#define MI355ZK_DEVOP_CHAIN 0x100
int mi355zk_selftest_dev_op(int op, int which, const uint32_t *in, size_t in_words_per_case, uint32_t *out, size_t out_words_per_case, size_t n_cases);

/* ---- mode / flag bits of the scalar-multiplication entry points below (batch_exp: `mode`; point_fft: `mode`; sparse_matvec: `flags`).
 * batch_exp and sparse_matvec return, by default, the reference's result for EVERY record the reference's decoders admit (point_fft: for
 * G2 records on the twist -- in the subgroup or not -- and G1 records on the curve; its stage kernels do not carry batch_exp's handling of
 * records on no curve, whose sums have no order-independent meaning anyway): the reference's `mul` is a wNAF
 * double-and-add (pairing/src/wnaf.rs:4-71, ec.rs:538-560, 983-997), i.e. the plain group law, and its bn256 decoders test the curve
 * equation at most (ec.rs:133-150, 1136-1344) -- never membership in the order-r subgroup of the twist -- while `compute_constrained`
 * reads its challenge unchecked (powersoftau/src/bin/compute_constrained.rs:16).  The G2 kernels therefore run PLAIN fixed windows over
 * the whole scalar.  MI355ZK_G2_TRUSTED_SUBGROUP is the caller's PROMISE that every G2 record of the call lies in the order-r subgroup
 * (honest ceremony data does; mi355zk_bn254_g2_subgroup_check_dev establishes it for untrusted data): the kernels then split each
 * scalar over the twist's endomorphism psi (k P = k1 P + k2 psi(P), k1, k2 < 2^128; psi(P) = mu P holds in that subgroup only) and
 * run 1.3-1.4 x faster (profiles/r05_g2_exact_cost.json).  A broken promise is not detected: a record with a cofactor component then
 * yields a point that is not k P.  The bit is accepted and ignored by the G1 entry points: E(Fq) has prime order r, so G1's split over
 * phi(x, y) = (beta x, y) is exact for every point ON the curve. */
#define MI355ZK_EXP_SAME_SCALAR 1      /* batch_exp: ONE scalar for all points (phase2 contribute) instead of one per point */
#define MI355ZK_FFT_INVERSE 1          /* point_fft: omega^-1 and the 1/m scaling */
#define MI355ZK_G2_TRUSTED_SUBGROUP 2  /* all three: the promise above */

/* ---- QAP evaluation: the per-variable sparse sums of MPCParameters::new
 * (phase2/src/parameters.rs:225-294: `a_g1[v] += coeffs_g1[lag].mul(coeff)` over the terms of variable v, then
 * batch_normalization) as one CSR-matrix x point-vector product:
 *   out[r] = sum_{t = row_ptr[r]}^{row_ptr[r+1]-1} coeff[t] * bases[col[t]],  r < n_rows,  affine out (all-zero = infinity).
 * row_ptr: u32[n_rows + 1] (row_ptr[n_rows] == nnz), col: u32[nnz], coeff: nnz canonical FrRepr; all device pointers.
 * The index arrays are validated on the device (col[t] < n_bases, row_ptr monotone from 0 to nnz): 3 = bad arguments otherwise.
 * `ext` of the reference (three products added) is one call on the concatenated term lists / bases.
 * flags: 0 or MI355ZK_G2_TRUSTED_SUBGROUP (other bits: 3 = bad arguments).  Synchronises `stream` before returning. */
int mi355zk_bn254_g1_sparse_matvec_dev(void *d_out_affine, const void *d_bases_affine, size_t n_bases, const uint32_t *d_row_ptr,
                                       const uint32_t *d_col, const void *d_coeffs, size_t n_rows, size_t nnz, void *stream, int flags);
int mi355zk_bn254_g2_sparse_matvec_dev(void *d_out_affine, const void *d_bases_affine, size_t n_bases, const uint32_t *d_row_ptr,
                                       const uint32_t *d_col, const void *d_coeffs, size_t n_rows, size_t nnz, void *stream, int flags);

/* The same on HOST buffers, over the device set of mi355zk_init (MPCParameters::new in one process on N GPUs): the rows are independent,
 * so device d evaluates the d-th contiguous row range -- its slice of (col, coeff), the whole base vector -- and writes its rows; no
 * exchange.  Same validation (3 = bad arguments) and output as the _dev form.  Synchronous. */
int mi355zk_bn254_g1_sparse_matvec(uint8_t *out_affine, const uint8_t *bases_affine, size_t n_bases, const uint32_t *row_ptr, const uint32_t *col,
                                   const uint64_t *coeffs, size_t n_rows, size_t nnz, int flags);
int mi355zk_bn254_g2_sparse_matvec(uint8_t *out_affine, const uint8_t *bases_affine, size_t n_bases, const uint32_t *row_ptr, const uint32_t *col,
                                   const uint64_t *coeffs, size_t n_rows, size_t nnz, int flags);

/* ---- point codecs: the reference's wire encodings <-> raw affine records.
 * Replaces EncodedPoint::{into_affine, into_affine_unchecked, from_affine} for G1Uncompressed (64 B), G1Compressed
 * (32 B), G2Uncompressed (128 B), G2Compressed (64 B)  (pairing/src/bn256/ec.rs:763-946, 1136-1344), which
 * powersoftau applies to every element of an accumulator file (batched_accumulator.rs read_points_chunk /
 * write_point): big-endian canonical coordinates, Fq2 as c1 || c0, byte 0 bit 7 = "y is the larger root"
 * (compressed), bit 6 = infinity.  n records, device pointers (byte buffers 4-byte aligned), one record per point;
 * the all-zero raw record is the point at infinity.  checked != 0: into_affine (on-curve test for uncompressed
 * input; decompression is on the curve by construction -- for G2 up to the reference's Fq2::sqrt quirk, which is
 * reproduced).  decode returns 0, or the GroupDecodingError of the FIRST failing record with its index in
 * *err_index (may be NULL): 4 NotOnCurve, 6 CoordinateDecodingError, 7 UnexpectedCompressionMode,
 * 8 UnexpectedInformation; failing records decode to infinity.  decode synchronises `stream`; encode is asynchronous. */
int mi355zk_bn254_g1_decode_dev(void *d_out_affine, const void *d_in_bytes, size_t n, int compressed, int checked, void *stream,
                                long long *err_index);
int mi355zk_bn254_g2_decode_dev(void *d_out_affine, const void *d_in_bytes, size_t n, int compressed, int checked, void *stream,
                                long long *err_index);
int mi355zk_bn254_g1_encode_dev(void *d_out_bytes, const void *d_in_affine, size_t n, int compressed, void *stream);
int mi355zk_bn254_g2_encode_dev(void *d_out_bytes, const void *d_in_affine, size_t n, int compressed, void *stream);

/* ---- FFT over curve points: EvaluationDomain<Point<G1>>::fft / ifft (bellman/src/group.rs:22-51
 * under domain.rs:154-173), the Lagrange-basis conversion of powersoftau/src/bin/prepare_phase2.rs:68-131.  In
 * place on 2^log_n AFFINE raw records (64 B, all-zero = infinity); the output is normalised to affine, i.e. what
 * `batch_normalization` + `into_affine` leave (ec.rs:251-299, 596-629).  mode: MI355ZK_FFT_INVERSE (omega^-1 and the 1/m scaling)
 * | MI355ZK_G2_TRUSTED_SUBGROUP; other bits: 3 = bad arguments.  Synchronises `stream` before returning. */
int mi355zk_bn254_g1_point_fft_dev(void *d_points_affine, uint32_t log_n, int mode, void *stream);
/* the same over G2 (128-byte affine records; `coeffs_g2` of prepare_phase2.rs:102-105): exact for every vector of points of the twist
 * (plain windows) unless the caller promises the subgroup */
int mi355zk_bn254_g2_point_fft_dev(void *d_points_affine, uint32_t log_n, int mode, void *stream);

/* ---- batch fixed-base scalar multiplication out[i] = k[i] * P, affine (all-zero = infinity).
 * Building block of the per-point `batch_exp` path (powersoftau/src/batched_accumulator.rs:1130-1181,
 * SURVEY 8f row 1); used here to synthesise tau-table-like bases on the device. */
int mi355zk_bn254_g1_batch_mul_dev(void *d_out_affine, const uint64_t base_affine[8], const void *d_scalars, size_t n, void *stream);
int mi355zk_bn254_g2_batch_mul_dev(void *d_out_affine, const uint64_t base_affine[16], const void *d_scalars, size_t n, void *stream);
/* ---- fixed-base scalar multiplication over a WINDOW TABLE of one base: out[i] = k[i] * P with no doubling per scalar.  The generator of
 * groth16/generator.rs:178-510 multiplies ONE generator by a scalar per variable (:406-426) and per H coefficient (:288-296) through
 * `Wnaf::base(..).scalar(..)` tables; batch_mul_dev above runs a whole variable-base multiplication (~254 doublings + ~66 additions) for
 * each.  Here the table holds (j * 2^(8 w)) * P for the 32 signed 8-bit windows w and j = 1 .. 128 (4096 affine entries), and a scalar costs
 * at most 32 mixed additions.  The entry format is the library's own: allocate mi355zk_fixed_base_table_bytes(group) bytes (1 = G1, 2 = G2;
 * 0 for anything else) and treat them as opaque.
 * build: one-time work, SYNCHRONISES `stream`; the 4096 entries come from the per-point batch_exp kernels over the scalars j * 2^(8 w) mod r.
 *   That reduction is sound in the order-r group only, so the base must be a non-infinite point of it -- G1: on the curve; G2: passing the
 *   membership test of mi355zk_bn254_g2_subgroup_check_dev (run on the host here).  3 (before any device work) = a NULL pointer, table_bytes
 *   too small, the all-zero record, a record off the curve, a twist point outside the subgroup.
 * mul: d_scalars = n canonical FrRepr (32 B each), or n Montgomery Fr with MI355ZK_FIXED_SCALARS_MONTGOMERY in `flags` (the kernel applies
 *   into_repr first, so Fr results feed it without a separate pass); out[i] = the affine record of k[i] * P, all-zero = infinity, which is
 *   what k = 0 gives.  A scalar >= r gives an UNSPECIFIED record for that element only: nothing faults, nothing outside the table is read,
 *   the other records are exact.  Asynchronous on `stream`; n == 0 succeeds and launches nothing.  d_table: a table built by the call above
 *   for the same group (not checked).  3 = a NULL pointer with n > 0, unknown flag bits, n >= 2^31. */
#define MI355ZK_FIXED_SCALARS_MONTGOMERY 1u
size_t mi355zk_fixed_base_table_bytes(int group);
int mi355zk_bn254_g1_fixed_base_build_dev(void *d_table, size_t table_bytes, const uint64_t base_affine[8], void *stream);
int mi355zk_bn254_g2_fixed_base_build_dev(void *d_table, size_t table_bytes, const uint64_t base_affine[16], void *stream);
int mi355zk_bn254_g1_fixed_base_mul_dev(void *d_out_affine, const void *d_table, const void *d_scalars, size_t n, uint32_t flags, void *stream);
int mi355zk_bn254_g2_fixed_base_mul_dev(void *d_out_affine, const void *d_table, const void *d_scalars, size_t n, uint32_t flags, void *stream);
/* ---- linear combinations over a SET of fixed G1 bases: out[i] = first + sum_{j < n_bases} k[i][j] * P_j, i < n, affine (all-zero =
 * infinity).  The input accumulators ic[0] + sum_j x_j ic[j + 1] of groth16/verifier.rs:44-48 for n proofs against one verifying key are one
 * call, one lane per proof; so is a single combination over many bases (n = 1), cut into slices of bases over many lanes.
 * A table set is n_bases tables of the geometry above laid end to end (table j starts at entry j * 4096): mi355zk_fixed_bases_table_bytes(n_bases)
 * bytes, 0 when that count cannot be served (n_bases * 4096 >= 2^31).
 * build: bases_affine = n_bases x 8 u64 in HOST memory.  One-time work, SYNCHRONISES `stream`; one batch_exp over all n_bases * 4096 entries.
 *   The all-zero record (the identity) is a base like any other: its table is all zero and contributes nothing.  n_bases == 0 succeeds and
 *   touches nothing.  3 (before any device work) = a NULL pointer, table_bytes too small, a base off the curve.
 * lincomb: d_scalars = n x n_bases canonical FrRepr, row-major (a scalar >= r: that row is unspecified, as above); d_first_affine = ONE
 *   device record, or NULL for the identity.  A lane serves one (row, slice of slice_len consecutive bases) and runs the fixed-base program
 *   once per base into one accumulator, through the general additions: a partial sum that equals the entry added, its negative, or the
 *   identity is handled.  With one slice the lane adds `first` itself; with several, the slices' sums go through stream-ordered scratch
 *   and a second kernel adds them per row.  slice_len == 0: the plan below; any other value is taken as given (clamped to n_bases).
 *   Asynchronous on `stream`, at most 2^18 lanes per launch; n == 0 succeeds and launches nothing; n_bases == 0 gives `first` n times.
 *   3 = a NULL pointer with work to do, n >= 2^31, n times the slice count >= 2^31.
 * plan: host arithmetic.  slice_len >= 1 and n_slices = ceil(n_bases / slice_len) (0 for n_bases == 0): no more slices than bring n * n_slices
 *   to MI355ZK_FIXED_BASES_LANE_TARGET lanes (ONE slice whenever n alone reaches the target), and no slice shorter than
 *   sqrt(n_bases / 16) bases, where a lane's walk over its slice and the join's walk over the slices take equally long.
 *   3 = a NULL pointer, n >= 2^31.  Both figures are measured: profiles/verify_proofs.md. */
#define MI355ZK_FIXED_BASES_LANE_TARGET 262144u
size_t mi355zk_fixed_bases_table_bytes(size_t n_bases);
int mi355zk_fixed_bases_plan(size_t n, size_t n_bases, size_t *slice_len, size_t *n_slices);
int mi355zk_bn254_g1_fixed_bases_build_dev(void *d_tables, size_t table_bytes, const uint64_t *bases_affine, size_t n_bases, void *stream);
int mi355zk_bn254_g1_fixed_bases_lincomb_dev(void *d_out_affine, const void *d_tables, size_t n_bases, const void *d_first_affine,
                                             const void *d_scalars, size_t n, size_t slice_len, void *stream);
/* ---- per-point batch exponentiation out[i] = k[i] * P[i] (powersoftau `batch_exp`, batched_accumulator.rs:1130-1181) or, with
 * MI355ZK_EXP_SAME_SCALAR in `mode`, out[i] = k[0] * P[i] (phase2 contribute, phase2/src/parameters.rs:423-470), normalised to affine
 * like `batch_normalization` (ec.rs:251-299); the all-zero record is infinity on both sides.  mode: MI355ZK_EXP_SAME_SCALAR |
 * MI355ZK_G2_TRUSTED_SUBGROUP (other bits: 3 = bad arguments).  Asynchronous on `stream`.
 * G2 is the reference's `mul` for every record -- in the subgroup, on the twist outside it, or (checked = 0 decoding) on no curve at
 * all: the plain windows are the group law of y^2 = x^3 + (y0^2 - x0^3), which no formula names.  G1 likewise: the split kernels test
 * y^2 = x^3 + 3 per record and hand an off-curve record (checked = 0 decoding only) to the plain-window kernel, so batch_exp returns the
 * reference's `mul` for those too (tests/test_g2_subgroup.py::test_batch_exp_of_records_that_are_on_no_curve). */
int mi355zk_bn254_g1_batch_exp_dev(void *d_out_affine, const void *d_bases_affine, const void *d_scalars, size_t n, int mode, void *stream);
int mi355zk_bn254_g2_batch_exp_dev(void *d_out_affine, const void *d_bases_affine, const void *d_scalars, size_t n, int mode, void *stream);
/* The same on HOST buffers, spread over the device set of mi355zk_init: what MPCParameters::contribute (parameters.rs:423-470) and
 * powersoftau's batch_exp (batched_accumulator.rs:1130-1181) are to a single-process caller.  The points are independent, so device d takes
 * the d-th contiguous point range -- upload, kernels, download from its own host thread, no exchange -- and with one device the
 * vector is one range.  out / bases: n raw affine records (64 / 128 B, all-zero = infinity; out may not alias bases); scalars: n canonical
 * FrRepr, or ONE with MI355ZK_EXP_SAME_SCALAR.  Synchronous.  mode as above. */
int mi355zk_bn254_g1_batch_exp(uint8_t *out_affine, const uint8_t *bases_affine, const uint64_t *scalars, size_t n, int mode);
int mi355zk_bn254_g2_batch_exp(uint8_t *out_affine, const uint8_t *bases_affine, const uint64_t *scalars, size_t n, int mode);
/* The test that lets a caller give the promise MI355ZK_G2_TRUSTED_SUBGROUP for data it did not produce: *bad_index = the lowest index of a G2 record that is on the twist but NOT in
 * the order-r subgroup (-1: all n records are; the all-zero record is the identity).  [x + 1] P + psi([x] P) + psi^2([x] P) == psi^3([2 x] P)
 * with x the 63-bit BN parameter -- one plain double-and-add (no split), sound and complete for BN254; a record that is not on the twist is not a member.  The reference has no counterpart -- its bn256 decoders do not test membership either -- so this
 * is an addition for callers that handle untrusted G2 data, not a drop-in for anything.  Synchronises `stream`. */
int mi355zk_bn254_g2_subgroup_check_dev(const void *d_points_affine, size_t n, void *stream, long long *bad_index);
int mi355zk_selftest_g2_in_subgroup(const uint64_t affine_pt[16]);   /* host run of the same test: 1 / 0 */

/* ---- powers-of-tau accumulator files, streamed: WIRE records in host memory on both sides (typically mmap'ed file ranges: pageable, `in`
 * may be read-only), decoded and encoded on the device, worked off in pieces so that device memory does not grow with n.  `in` / `out` hold
 * n records of 64 / 128 B (G1 / G2 uncompressed) or 32 / 64 B (compressed), the encodings of the point codecs above.
 * piece: records per device piece (0 = 2^18).  Piece i + 1 is uploaded while piece i runs its kernels and piece i - 1 is downloaded (two
 * buffer sets, a copy and a compute stream of the calling thread's current device).  Device memory of a call, with P = min(piece, n):
 *   transform    2 P (in_record + out_record + 2 raw + 32) B + batch_exp's own scratch for P points
 *   power_pairs  2 P (in_record + raw + out_record or 0 + 1) B + P 32 B of exponents + the dense multiexp's pools for P points
 * (raw = 64 / 128 B), never a function of n.
 * accumulator_transform: out[i] = encode((coeff * tau^(first + i)) * decode(in[i])) -- the body of BatchedAccumulator::transform for one
 *   vector range (powersoftau/src/batched_accumulator.rs:1187-1290: read_chunk, taupowers, batch_exp, the not-infinity assertion,
 *   write_chunk).  tau, coeff: canonical FrRepr (< r, else 3); coeff == NULL is 1.  checked: into_affine instead of into_affine_unchecked.
 *   mode: 0 or MI355ZK_G2_TRUSTED_SUBGROUP (as batch_exp; ignored for G1).  in and out may not overlap.
 * accumulator_power_pairs: decodes n records and returns the Jacobian sums s = sum_{i < n-1} rho_(first+i) v[i] and
 *   sx = sum_{i < n-1} rho_(first+i) v[i+1], rho_g = scalar g of the stream (key, stream_id) of fr_random above: power_pairs
 *   (powersoftau/src/utils.rs:133-135) over one chunk.  The scalar index is global, so the sums over chunks that overlap by one record add up
 *   (mi355zk_bn254_g{1,2}_add) to exactly what merge_pairs_random gives for the whole vector, however it is cut.  n == 1 gives two
 *   identities.  out_uncompressed (may be NULL): the n records re-encoded uncompressed in the same pass (`decompress`,
 *   batched_accumulator.rs:543-617).  check_subgroup (G2 only): every record must pass the test of mi355zk_bn254_g2_subgroup_check_dev.
 * Both: 3 = a NULL pointer, n >= 2^31, piece == 1; n == 0 succeeds and does nothing.  A record the decoder refuses returns the decoder's code
 * (4, 6, 7, 8), a G2 record outside the subgroup under check_subgroup 5, a point at infinity on input -- or on transform's output --
 * MI355ZK_ERR_POINT_AT_INFINITY (read_points_chunk :938-983, :1176); *err_index (may be NULL) is then the lowest index, within the call, of
 * the pieces up to the first that fails, and -1 otherwise.  On any non-zero return the contents of `out` / `out_uncompressed` are unspecified
 * (the caller discards the file).  Synchronous; re-entrant from several host threads. */
int mi355zk_bn254_g1_accumulator_transform(uint8_t *out, const uint8_t *in, size_t n, uint64_t first, const uint64_t tau[4], const uint64_t coeff[4],
                                           int in_compressed, int out_compressed, int checked, uint32_t mode, size_t piece, long long *err_index);
int mi355zk_bn254_g2_accumulator_transform(uint8_t *out, const uint8_t *in, size_t n, uint64_t first, const uint64_t tau[4], const uint64_t coeff[4],
                                           int in_compressed, int out_compressed, int checked, uint32_t mode, size_t piece, long long *err_index);
int mi355zk_bn254_g1_accumulator_power_pairs(const uint8_t *in, size_t n, int compressed, int checked, int check_subgroup, const uint32_t key[8],
                                             uint64_t stream_id, uint64_t first, uint8_t *out_uncompressed, size_t piece, uint64_t out_s[12],
                                             uint64_t out_sx[12], long long *err_index);
int mi355zk_bn254_g2_accumulator_power_pairs(const uint8_t *in, size_t n, int compressed, int checked, int check_subgroup, const uint32_t key[8],
                                             uint64_t stream_id, uint64_t first, uint8_t *out_uncompressed, size_t piece, uint64_t out_s[24],
                                             uint64_t out_sx[24], long long *err_index);

/* ---- whole vectors between a file and the device: n WIRE records in host memory (typically an mmap'ed file range, pageable, `in` may be
 * read-only) <-> n raw affine records (64 / 128 B) in the CALLER's device vector, which stays on the device for the transforms that follow
 * (powersoftau/src/bin/prepare_phase2.rs reads each accumulator vector once and writes its Lagrange form for every degree).  The work runs in
 * pieces of `piece` records (0 = 2^18) over two buffer sets, a copy and a compute stream of the calling thread's current device: the upload
 * (download) of one piece overlaps the decoding (encoding) of the next.  Device memory beyond the caller's vector, with P = min(piece, n):
 *   points_load   2 (P (in_record + 1 under check_subgroup) + 256) B     points_store   2 P out_record B
 * (each term rounded up to 256 B), never a function of n; in_record / out_record = 64 / 128 B uncompressed, 32 / 64 B compressed.
 * points_load: d_out[i] = decode(in[i]) with the codec kernels above (checked: into_affine instead of into_affine_unchecked).  A record the
 *   decoder refuses returns the decoder's code (4, 6, 7, 8), an all-zero decoded record MI355ZK_ERR_POINT_AT_INFINITY (read_points_chunk,
 *   batched_accumulator.rs:938-983), under check_subgroup (G2 only; ignored for G1) a record outside the order-r subgroup 5; *err_index (may
 *   be NULL) is then the lowest such index, within the call, of the first piece that fails -- later pieces are not looked at -- and -1
 *   otherwise.  Within a piece the order is: decoding, infinity, membership.  On a non-zero return the contents of d_out are unspecified.
 * points_store: out[i] = encode(d_in[i]); the all-zero record is written as the codec writes infinity.
 * Both: 3 = a NULL pointer with n > 0, a device pointer that is not 16-byte aligned, piece >= 2^31; n == 0 succeeds and does nothing.
 * Synchronous: they return after the last piece has completed, and they do NOT order themselves after work queued on any other stream -- the
 * caller synchronises the stream that produced d_in (or will consume d_out) itself.  Re-entrant from several host threads. */
int mi355zk_bn254_g1_points_load(void *d_out_affine, const uint8_t *in, size_t n, int compressed, int checked, int check_subgroup, size_t piece,
                                 long long *err_index);
int mi355zk_bn254_g2_points_load(void *d_out_affine, const uint8_t *in, size_t n, int compressed, int checked, int check_subgroup, size_t piece,
                                 long long *err_index);
int mi355zk_bn254_g1_points_store(uint8_t *out, const void *d_in_affine, size_t n, int compressed, size_t piece);
int mi355zk_bn254_g2_points_store(uint8_t *out, const void *d_in_affine, size_t n, int compressed, size_t piece);

/* ---- the H bases of prepare_phase2.rs:137-147: out[i] = in[i + shift] - in[i], i < n_out, on raw affine G1 records (64 B, all-zero =
 * infinity); the output is affine and normalised, byte for byte what the two-term rows of mi355zk_bn254_g1_sparse_matvec_dev give, without
 * their index and coefficient arrays (72 B per output).  One affine chord per output -- the tangent at in[i + shift] when
 * in[i + shift] == -in[i], infinity when the two are equal, the other operand (negated for in[i]) when one is infinity -- and one field
 * inversion per MI355ZK_SHIFTED_DIFFERENCE_K consecutive outputs.  No device memory beyond the two vectors.  DOMAIN: points on the curve;
 * nothing is tested and nothing faults outside it.  Asynchronous on `stream`.
 * 3 = shift == 0, shift + n_out > n_in, out[0, n_out) overlapping in[0, n_in), and with n_out > 0 a NULL or not 16-byte aligned pointer;
 * n_out == 0 succeeds and launches nothing.  There is no G2 twin: the H bases are G1 only.
 * mi355zk_selftest_g1_shifted_difference: the same lane routine, with the same grouping into shared inversions, run on HOST records (no
 * device needed; 8-byte alignment suffices). */
#define MI355ZK_SHIFTED_DIFFERENCE_K 16
int mi355zk_bn254_g1_shifted_difference_dev(void *d_out_affine, const void *d_in_affine, size_t n_in, size_t shift, size_t n_out, void *stream);
int mi355zk_selftest_g1_shifted_difference(uint64_t *out, const uint64_t *in, size_t n_in, size_t shift, size_t n_out);

/* ---- the pairing e: G1 x G2 -> GT (Engine::miller_loop + final_exponentiation, pairing/src/bn256/mod.rs:57-226) in its batched form: many
 * independent pairing PRODUCTS in one call -- every same_ratio of a verify_transformation (powersoftau/src/utils.rs:151-159), the four
 * pairings per contribution of MPCParameters::verify (phase2/src/parameters.rs:529-659), the three-pair product of each of many proofs
 * (bellman/src/groth16/verifier.rs:36-67).  One lane runs one Miller loop; a segmented product joins the values of a group; one lane per
 * group runs the final exponentiation.
 * Points: raw affine records, 64 B (G1) / 128 B (G2), the all-zero record = infinity; a pair with one contributes the value one (mod.rs:68).
 * DOMAIN: G1 points on the curve, G2 points on the twist AND in the order-r subgroup.  Like the reference, the library tests neither;
 * outside the domain the values are unspecified and nothing faults.  mi355zk_bn254_g2_subgroup_check_dev establishes it for untrusted G2 data.
 * A GT value is 384 B: twelve Fq as Montgomery u64[4] limbs in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 (Fq12 -> Fq6 -> Fq2 ->
 * Fq, the reference's struct order).  After the final exponentiation it is a unique, fully reduced field element: equal values are equal
 * bytes, here and in the reference. */
/* out[g] = final_exponentiation( prod_{i in [group_ptr[g], group_ptr[g+1])} miller(P_i, Q_i) ), 384 B each; an empty group gives one.
   d_group_ptr: n_groups + 1 uint32 on the device, nondecreasing from 0 to n_pairs.  It is NOT checked (it is the caller's device data):
   entries are clamped to n_pairs, so a bad array gives unspecified values and no access out of range.
   d_group_ptr == NULL: every pair is its own group (n_groups must equal n_pairs).  Asynchronous on `stream`; n_groups == 0 succeeds and
   launches nothing.  The Miller values live in one stream-ordered allocation of 384 B per pair, released on `stream` by the call itself.
   3 = NULL pointer with n > 0, n_pairs or n_groups >= 2^31, d_group_ptr == NULL with n_groups != n_pairs. */
int mi355zk_bn254_pairing_product_dev(void *d_gt_out, const void *d_g1_affine, const void *d_g2_affine, size_t n_pairs,
                                      const uint32_t *d_group_ptr, size_t n_groups, void *stream);
/* flags[g] = 1 iff gt[g] is one / iff gt_a[g] == gt_b[g] (bytes); for callers that want booleans only.  Asynchronous on `stream`. */
int mi355zk_bn254_gt_is_one_dev(uint8_t *d_flags, const void *d_gt, size_t n, void *stream);
int mi355zk_bn254_gt_eq_dev(uint8_t *d_flags, const void *d_gt_a, const void *d_gt_b, size_t n, void *stream);
/* the same product for ONE group on the host, single thread, no device needed (the same arithmetic compiled for the host): the
   once-per-key pairing of prepare_verifying_key (verifier.rs:19-34).  n_pairs == 0 gives one.  3 = NULL pointer, n_pairs >= 2^31. */
int mi355zk_bn254_pairing_product(uint64_t gt_out[48], const uint64_t *g1_affine, const uint64_t *g2_affine, size_t n_pairs);
/* one tower primitive on the host.  Operands and result are Fq12 (48 words), Fq6 (24) or Fq2 (8) in the formats above, concatenated in
   `in` in the order given; in_words / out_words must be exactly the op's (3 otherwise, as for an unknown op or a NULL pointer):
     FQ6_MUL a b -> a b          FQ6_INV a -> 1 / a (0 for 0)       FQ6_MUL_BY_01 a b0 b1 -> a (b0 + b1 v)      FQ6_MUL_BY_1 a b1 -> a b1 v
     FQ12_MUL a b -> a b         FQ12_SQR a -> a^2                  FQ12_INV a -> 1 / a (0 for 0)               FQ12_CONJUGATE a -> a^(q^6)
     FQ12_FROBENIUS_k a -> a^(q^k), k = 1, 2, 3                     FQ12_MUL_BY_034 a c0 c3 c4 -> a (c0 + (c3 + c4 v) w)
     FINAL_EXPONENTIATION a -> a^((q^12 - 1) / r) */
#define MI355ZK_PAIRING_OP_FQ6_MUL 0
#define MI355ZK_PAIRING_OP_FQ6_INV 1
#define MI355ZK_PAIRING_OP_FQ6_MUL_BY_01 2
#define MI355ZK_PAIRING_OP_FQ6_MUL_BY_1 3
#define MI355ZK_PAIRING_OP_FQ12_MUL 4
#define MI355ZK_PAIRING_OP_FQ12_SQR 5
#define MI355ZK_PAIRING_OP_FQ12_INV 6
#define MI355ZK_PAIRING_OP_FQ12_CONJUGATE 7
#define MI355ZK_PAIRING_OP_FQ12_FROBENIUS_1 8
#define MI355ZK_PAIRING_OP_FQ12_FROBENIUS_2 9
#define MI355ZK_PAIRING_OP_FQ12_FROBENIUS_3 10
#define MI355ZK_PAIRING_OP_FQ12_MUL_BY_034 11
#define MI355ZK_PAIRING_OP_FINAL_EXPONENTIATION 12
int mi355zk_selftest_pairing_op(int op, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words);

/* ---- host-side group helpers on Jacobian results: acc += other (CurveProjective::add_assign,
 * ec.rs:360-454) -- how per-GPU partial sums are joined after the all-gather -- and into_affine
 * (ec.rs:596-629; infinity -> all-zero record). */
int mi355zk_bn254_g1_add(uint64_t acc_xyz[12], const uint64_t other_xyz[12]);
int mi355zk_bn254_g2_add(uint64_t acc_xyz[24], const uint64_t other_xyz[24]);
int mi355zk_bn254_g1_to_affine(uint64_t out_xy[8], const uint64_t xyz[12]);
int mi355zk_bn254_g2_to_affine(uint64_t out_xy[16], const uint64_t xyz[24]);
/* acc = scalar * acc on the host (CurveProjective::mul_assign, ec.rs:538-560), scalar = 4 canonical u64 limbs: the single-point
 * products of a proof assembly (bellman/src/groth16/prover.rs:300-333). */
int mi355zk_bn254_g1_mul(uint64_t acc_xyz[12], const uint64_t scalar[4]);
int mi355zk_bn254_g2_mul(uint64_t acc_xyz[24], const uint64_t scalar[4]);

/* ---- plain device-memory helpers so that a C / Rust caller needs no HIP bindings of its own */
int mi355zk_malloc(void **d_ptr, size_t bytes);
int mi355zk_free(void *d_ptr);
int mi355zk_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int mi355zk_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);
int mi355zk_sync(void *stream);

/* ---- per-kernel timing (HIP events on the launch stream) for bench.py's roofline leg.
 * names: "msm_digits" "msm_sort" "msm_accumulate_heavy" "msm_accumulate" "msm_reduce" "ntt_pass" "ntt_scale"
 * mi355zk_prof_enable: 0 off; 1 every kernel group (~20 event records per multiexp: 0.1-0.2 ms of host time per call); 2 only the
 * group named by mi355zk_prof_only (two records per call: what bench.py leaves on inside its timed region, for the dominant kernel). */
void mi355zk_prof_enable(int on);
void mi355zk_prof_only(const char *kernel);
void mi355zk_prof_reset(void);
int mi355zk_prof_get(const char *kernel, double *total_ms, long *count);

#ifdef __cplusplus
}
#endif
#endif /* MI355ZK_H */
