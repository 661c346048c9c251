// Internal interfaces between the translation units of libmi355zk.so (not part of the C ABI: include/mi355zk.h is).
//   api.hip         the C ABI: argument checking, domain constants, device-resident entry points, profiling hooks, lifecycle
//   host_entry.hip  the multiexp behind the ABI: device-resident call wrapper, streamed upload of a host-buffer call, multi-GPU cells
//   host_ops.hip    the other host-buffer entry points: batch_exp, dense multiexp / merge_pairs, NTT, H polynomial, QAP sparse matvec
//   host_plan.hpp   what those two plan, without a device: Source / Density arithmetic, chunk schedule, cells and their join, row cuts, knobs
//   bases_cache.hip the pinned-bases cache (bases_cache.hpp: its interface; the entries and their lock are its own)
//   host_pools.hip  the stage pool and the device set (host_pools.hpp: leases, events, the fan-out over devices)
//   scalar_mul.hip  the scalar-multiplication kernels and their launchers: batch_exp / batch_mul / window-table build / G2 membership
//   fr_random.hip   the random exponents of merge_pairs generated on the device (chacha.hpp: the generator shared with the host)
//   accumulator_stream.hip  powers-of-tau files streamed through the device: wire records in host memory on both sides, bounded pieces
//   point_diff.hip  out[i] = in[i + shift] - in[i] on affine G1 records: the H bases of prepare_phase2 without index arrays
//   fixed_base.hip  one base, a window table of its multiples, no doublings per scalar (fixed_base.hpp: the program shared with the host);
//                   table sets over several G1 bases and linear combinations over them, sliced over lanes (the slice plan)
//   (msm_g1.hip, msm_g2.hip, msm_partition.hip, ntt.hip, point_fft*.hip, codec.hip, field_ops.hip, records.hip: the kernels behind the functions declared below)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "curveu.hpp"
#include "device_util.hpp"

namespace zk {
// ntt.hip
int ntt_run(Fr* d_a, uint32_t log_n, const Fr& omega, hipStream_t st);
int ntt_run_scaled(Fr* d_a, uint32_t log_n, const Fr& omega, const Fr* pre_g, const Fr* post_c, const Fr* post_g, hipStream_t st);
int ntt_run_batch(Fr* const* d_arrays, uint32_t batch, uint32_t log_n, const Fr& omega, const Fr* pre_g, const Fr* post_c, const Fr* post_g, hipStream_t st);
int ntt_scale(Fr* d_a, uint32_t log_n, const Fr& c, const Fr* g, hipStream_t st);
void ntt_release_all();
int ntt_configure();
// msm_g1.hip, msm_g2.hip (the kernels: msm_impl.hpp; msm_device: msm_host.hpp); the geometry and self-test functions: msm_partition.hip
int msm_g1_device(const void* d_bases, uint64_t n_bases, uint64_t base_offset, const void* d_scalars, uint64_t n, const uint32_t* d_density,
                  const uint32_t* d_dprefix, hipStream_t st, uint64_t out_xyz[12], long long* err_index, uint32_t wgroups, uint32_t wgroup, bool scalars_mont,
                  MsmChunks* chunks, uint64_t table_stride = 0, uint32_t table_c = 0);
void msm_table_geometry(uint64_t n_bases, int group, uint32_t* c, uint32_t* W, uint8_t width[64]);
int msm_g2_device(const void* d_bases, uint64_t n_bases, uint64_t base_offset, const void* d_scalars, uint64_t n, const uint32_t* d_density,
                  const uint32_t* d_dprefix, hipStream_t st, uint64_t out_xyz[24], long long* err_index, uint32_t wgroups, uint32_t wgroup, bool scalars_mont,
                  MsmChunks* chunks, uint64_t table_stride = 0, uint32_t table_c = 0);
// n_vectors exponent vectors over one base vector and one density map in one pipeline (msm_host.hpp: msm_device_batch); per-vector codes in rcs / err_indices
int msm_g1_batch_device(const void* d_bases, uint64_t n_bases, uint64_t base_offset, const void* d_scalars, uint64_t n, uint64_t scalar_stride,
                        uint32_t n_vectors, const uint32_t* d_density, const uint32_t* d_dprefix, hipStream_t st, uint64_t* out_xyz, int* rcs,
                        long long* err_indices, bool scalars_mont);
int msm_g2_batch_device(const void* d_bases, uint64_t n_bases, uint64_t base_offset, const void* d_scalars, uint64_t n, uint64_t scalar_stride,
                        uint32_t n_vectors, const uint32_t* d_density, const uint32_t* d_dprefix, hipStream_t st, uint64_t* out_xyz, int* rcs,
                        long long* err_indices, bool scalars_mont);
int msm_g1_dense_device(const void* d_bases, const void* d_bases2, const void* d_scalars, uint64_t n, hipStream_t st, uint64_t* out_xyz, uint64_t* out2_xyz);
int msm_g1_buckets_device(const void* d_bases, const void* d_scalars, uint64_t n, hipStream_t st, uint64_t out_xyz[12], uint32_t* n_buckets, uint32_t* n_vals,
                          uint32_t* first, uint32_t* last, size_t cap_buckets, uint32_t* vals, size_t cap_vals, uint64_t* records);
int msm_g2_dense_device(const void* d_bases, const void* d_bases2, const void* d_scalars, uint64_t n, hipStream_t st, uint64_t* out_xyz, uint64_t* out2_xyz);
int segsum_g1_device(const void* d_points, uint64_t nnz, const uint32_t* d_row_ptr, uint32_t n_rows, hipStream_t st, void* d_out);
int segsum_g2_device(const void* d_points, uint64_t nnz, const uint32_t* d_row_ptr, uint32_t n_rows, hipStream_t st, void* d_out);
void msm_release_g1();
void msm_release_g2();
void msm_geometry(uint64_t n, uint32_t wgroups, uint32_t* c, uint32_t* W);
void msm_batch_geometry(uint64_t n, uint32_t n_vectors, int group, uint32_t* max_windows, uint32_t* W, uint32_t* vectors_per_pass);   // MSM_BATCH_MAX_WINDOWS, windows of one vector, msm_batch_split
int msm_selftest_digits(uint64_t n, uint32_t wgroups, const uint32_t scalar[8], uint32_t w_start, uint32_t w_stop, int direct, int32_t* digits,
                        uint32_t* geom);
// point_fft.hip
int point_fft_g1(void* d_points, uint32_t log_n, const Fr& omega, bool scale, const Fr& scale_canon, hipStream_t st);
// codec.hip
int codec_decode(int group, void* d_out, const void* d_in, size_t n, int compressed, int checked, hipStream_t st, long long* err_index);
int codec_encode(int group, void* d_out, const void* d_in, size_t n, int compressed, hipStream_t st);
// the decode kernel alone, enqueued on `st`: *d_err (set to ~0 by the caller, on the stream) takes the minimum of (index << 8 | code) over the refused records
int codec_decode_enqueue(int group, void* d_out, const void* d_in, size_t n, int compressed, int checked, hipStream_t st, unsigned long long* d_err);
// point_fft_g2.hip
int point_fft_g2(void* d_points, uint32_t log_n, const Fr& omega, bool scale, const Fr& scale_canon, hipStream_t st, bool trusted_subgroup);

// scalar_mul.hip
// out[i] = k[i or 0] * P[i or base_index[i] or 0], affine (batched_accumulator.rs:1130-1181, parameters.rs:423-470); see the definition for the modes
template <class F>
int batch_exp(void* d_out, const void* d_bases, int same_base, const void* d_scalars, int same_scalar, size_t n, void* stream,
              const uint32_t* d_base_index = nullptr, bool shortcut_unit_scalars = false, bool g2_trusted = false,
              const uint8_t* d_g2_member = nullptr);
extern template int batch_exp<Fq>(void*, const void*, int, const void*, int, size_t, void*, const uint32_t*, bool, bool, const uint8_t*);
extern template int batch_exp<Fq2>(void*, const void*, int, const void*, int, size_t, void*, const uint32_t*, bool, bool, const uint8_t*);
template <class F>
int batch_mul(void* d_out, const uint64_t* base_raw, const void* d_scalars, size_t n, void* stream);
extern template int batch_mul<Fq>(void*, const uint64_t*, const void*, size_t, void*);
extern template int batch_mul<Fq2>(void*, const uint64_t*, const void*, size_t, void*);
template <int GROUP>
int msm_table_build(const void* d_bases, size_t n, void* d_table, size_t table_bytes, void* stream);
extern template int msm_table_build<1>(const void*, size_t, void*, size_t, void*);
extern template int msm_table_build<2>(const void*, size_t, void*, size_t, void*);
int g2_subgroup_flags(const void* d_points, size_t n, void* stream, uint8_t* d_member);
int g2_subgroup_check(const void* d_points, size_t n, void* stream, long long* bad_index);
bool g2_in_subgroup_host(const Affine<Fq2>& p);   // the membership test of the kernels, run on the host (self-test hook)
bool g1_on_curve_host(const Affine<Fq>& p);       // y^2 == x^3 + 3, as the split kernels test it
// the per-(device, stream) scratch of the scalar-multiplication launchers (Z coordinates between a kernel and its normalisation; grow-only) and
// the mutex their callers hold while ENQUEUEING: the kernels of one call must reach the stream back to back (see batch_exp)
int exp_scratch(size_t bytes, void* stream, void** out);
extern std::mutex g_exp_launch_mu;
int batch_normalize_g1(void* d_io_affine, const void* d_z, uint64_t n, hipStream_t st);
int batch_normalize_g2(void* d_io_affine, const void* d_z, uint64_t n, hipStream_t st);
void scalar_mul_release_all();   // the scratch above and batch_mul's slot rings

// records.hip: base vectors in the CALLER's record layout (bellman's `G1Affine { x, y, infinity: bool }` is 72 B, G2Affine 136 B).
// stride == 0 is the packed layout of the group (64 / 128 B, x || y, no flag).  Every non-packed layout passed below has been checked by
// records_layout_check (coordinate ranges inside the record, disjoint, 4-byte aligned; the flag byte outside them).
struct RecordLayout {
  size_t stride = 0, x_off = 0, y_off = 0, inf_off = (size_t)-1;
  bool packed() const { return stride == 0; }
  size_t host_stride(int group) const { return stride ? stride : (group == 1 ? 64 : 128); }
  bool operator==(const RecordLayout& o) const { return stride == o.stride && x_off == o.x_off && y_off == o.y_off && inf_off == o.inf_off; }
  bool operator!=(const RecordLayout& o) const { return !(*this == o); }
};
// the ABI's argument rules (include/mi355zk.h: rc 3) -> ZK_OK and *out (the packed layout normalised to stride 0), or ZK_ERR_BAD_ARGS
int records_layout_check(int group, size_t stride, size_t x_off, size_t y_off, size_t inf_off, RecordLayout* out);
// n raw records at d_raw -> n packed records at d_out (the records_pack kernel, enqueued on `st`; no synchronisation)
int records_pack_run(int group, const void* d_raw, size_t n, const RecordLayout& L, void* d_out, hipStream_t st);

// field_ops.hip
int fr_h_combine(Fr* d_a, const Fr* d_b, const Fr* d_c, size_t n, const Fr& zinv, hipStream_t st);   // a[i] = (a[i] * b[i] - c[i]) * zinv, one pass
int fr_mul_add(Fr* d_a, const Fr* d_b, const Fr& c, size_t n, hipStream_t st);                        // a[i] += c * b[i] (d_b NULL: a[i] += c)
int fr_into_repr(Fr* d_out, const Fr* d_in, size_t n, hipStream_t st);                                // Montgomery -> canonical (d_out may alias d_in)
int fr_powers(Fr* d_out, const Fr& base, const Fr& coeff, size_t n, hipStream_t st);               // out[i] = coeff * base^i (Montgomery)
// fr_poly.hip
void fr_poly_release_all();   // the per-(device, stream) scratch of the polynomial division / evaluation (mi355zk_shutdown)
// fr_scan.hip
void fr_scan_release_all();   // the tile aggregates of the prefix scans, per (device, stream)
// fr_inverse.hip, fr_evals.hip
void fr_inverse_release_all();   // the tile products of the batch inversion, per (device, stream)
void fr_evals_release_all();     // the omega table, the partial sums and the denominators of evals_divide, per (device, stream)

// fr_random.hip: scalars first .. first + n - 1 of the stream (key, stream_id) of chacha.hpp as canonical FrRepr at d_out (16-byte aligned), enqueued on `st`
struct FrRandomStream {
  uint32_t key[8];
  uint64_t stream_id;
};
int fr_random_fill(void* d_out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first, hipStream_t st);

// api.hip
int domain_op_dev(Fr* d_a, uint32_t log_n, int op, hipStream_t st);   // EvaluationDomain::{fft, ifft, coset_fft, icoset_fft} on a device array
int domain_op_batch_dev(Fr* const* d_arrays, uint32_t batch, uint32_t log_n, int op, hipStream_t st);
// the H polynomial of prover.rs:216-248 behind a, b, c in the coset evaluation form: h_combine, icoset_fft, into_repr (MI355ZK_H_INTO_REPR)
int h_poly_finish_dev(Fr* d_a, const Fr* d_b, const Fr* d_c, uint32_t log_n, uint32_t flags, hipStream_t st);

// host_entry.hip
extern thread_local long long t_last_err_index;   // exponent index of the last Source error of this thread's calls (mi355zk_last_error_index)
// the device-resident multiexp behind every _dev entry point (table: d_bases is a window table; chunks: exponents handed over while the call runs)
template <int GROUP>
int msm_dev_entry(const void* d_bases, size_t n_bases, size_t base_offset, const void* d_scalars, size_t n_scalars, const uint32_t* density,
                  size_t density_bits, void* stream, uint64_t* out_xyz, uint32_t wgroups = 1, uint32_t wgroup = 0, uint32_t flags = 0,
                  MsmChunks* chunks = nullptr, bool table = false);
// the batch entry (mi355zk_bn254_g{1,2}_msm_batch_dev): vector v's rc / exponent index as msm_dev_entry gives them for that vector alone
template <int GROUP>
int msm_batch_dev_entry(const void* d_bases, size_t n_bases, size_t base_offset, const void* d_scalars, size_t n_scalars, size_t scalar_stride,
                        size_t n_vectors, const uint32_t* density, size_t density_bits, uint32_t flags, void* stream, uint64_t* out_xyz, int* rcs,
                        long long* err_indices);
extern template int msm_batch_dev_entry<1>(const void*, size_t, size_t, const void*, size_t, size_t, size_t, const uint32_t*, size_t, uint32_t, void*, uint64_t*, int*, long long*);
extern template int msm_batch_dev_entry<2>(const void*, size_t, size_t, const void*, size_t, size_t, size_t, const uint32_t*, size_t, uint32_t, void*, uint64_t*, int*, long long*);
// host buffers: whole on one device (streamed upload, pinned-bases cache) or cut into cells over the device set of mi355zk_init
template <int GROUP>
int msm_host_entry(const uint8_t* bases, size_t n_bases, size_t base_offset, const uint64_t* scalars, size_t n_scalars, const uint32_t* density,
                   size_t density_bits, uint64_t* out_xyz, const RecordLayout& L = RecordLayout());
extern template int msm_dev_entry<1>(const void*, size_t, size_t, const void*, size_t, const uint32_t*, size_t, void*, uint64_t*, uint32_t, uint32_t, uint32_t, MsmChunks*, bool);
extern template int msm_dev_entry<2>(const void*, size_t, size_t, const void*, size_t, const uint32_t*, size_t, void*, uint64_t*, uint32_t, uint32_t, uint32_t, MsmChunks*, bool);
extern template int msm_host_entry<1>(const uint8_t*, size_t, size_t, const uint64_t*, size_t, const uint32_t*, size_t, uint64_t*, const RecordLayout&);
extern template int msm_host_entry<2>(const uint8_t*, size_t, size_t, const uint64_t*, size_t, const uint32_t*, size_t, uint64_t*, const RecordLayout&);
// host_ops.hip
template <class F>
int batch_exp_host(uint8_t* out, const uint8_t* bases, const uint64_t* scalars, size_t n, int same_scalar, bool g2_trusted);
// rnd != nullptr: rho is not read -- every piece fills its exponents on its device from the scalar stream of chacha.hpp, from the piece's first index
template <int GROUP>
int dense_host(const uint8_t* v1, const uint8_t* v2, const uint64_t* rho, size_t n, uint64_t* out_s, uint64_t* out_sx, const FrRandomStream* rnd = nullptr);
int ntt_host(uint64_t* a, uint32_t log_n, int op, const uint64_t* omega);
int h_poly_host(uint64_t* h, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t len, uint32_t log_n, uint32_t flags);
template <class F>
int sparse_matvec(void* d_out, const void* d_bases, size_t n_bases, const uint32_t* d_row_ptr, const uint32_t* d_col, const void* d_coeffs,
                  size_t n_rows, size_t nnz, void* stream, int group, bool g2_trusted, void* d_scratch = nullptr, size_t scratch_bytes = 0);
template <class F>
int sparse_matvec_host(uint8_t* out, const uint8_t* bases, size_t n_bases, const uint32_t* row_ptr, const uint32_t* col, const uint64_t* coeffs,
                       size_t n_rows, size_t nnz, int group, bool g2_trusted);
extern template int batch_exp_host<Fq>(uint8_t*, const uint8_t*, const uint64_t*, size_t, int, bool);
extern template int batch_exp_host<Fq2>(uint8_t*, const uint8_t*, const uint64_t*, size_t, int, bool);
extern template int dense_host<1>(const uint8_t*, const uint8_t*, const uint64_t*, size_t, uint64_t*, uint64_t*, const FrRandomStream*);
extern template int dense_host<2>(const uint8_t*, const uint8_t*, const uint64_t*, size_t, uint64_t*, uint64_t*, const FrRandomStream*);
extern template int sparse_matvec<Fq>(void*, const void*, size_t, const uint32_t*, const uint32_t*, const void*, size_t, size_t, void*, int, bool, void*, size_t);
extern template int sparse_matvec<Fq2>(void*, const void*, size_t, const uint32_t*, const uint32_t*, const void*, size_t, size_t, void*, int, bool, void*, size_t);
extern template int sparse_matvec_host<Fq>(uint8_t*, const uint8_t*, size_t, const uint32_t*, const uint32_t*, const uint64_t*, size_t, size_t, int, bool);
extern template int sparse_matvec_host<Fq2>(uint8_t*, const uint8_t*, size_t, const uint32_t*, const uint32_t*, const uint64_t*, size_t, size_t, int, bool);
// accumulator_stream.hip (include/mi355zk.h: mi355zk_bn254_g{1,2}_accumulator_transform / _power_pairs)
template <int GROUP>
int accumulator_transform(uint8_t* out, const uint8_t* in, size_t n, uint64_t first, const uint64_t* tau, const uint64_t* coeff, int in_compressed,
                          int out_compressed, int checked, uint32_t mode, size_t piece, long long* err_index);
template <int GROUP>
int accumulator_power_pairs(const uint8_t* in, size_t n, int compressed, int checked, int check_subgroup, const uint32_t* key, uint64_t stream_id,
                            uint64_t first, uint8_t* out_uncompressed, size_t piece, uint64_t* out_s, uint64_t* out_sx, long long* err_index);
// wire records in host memory <-> a whole vector of raw affine records on the device, in pieces (mi355zk_bn254_g{1,2}_points_load / _store)
template <int GROUP>
int points_load(void* d_out, const uint8_t* in, size_t n, int compressed, int checked, int check_subgroup, size_t piece, long long* err_index);
template <int GROUP>
int points_store(uint8_t* out, const void* d_in, size_t n, int compressed, size_t piece);
extern template int points_load<1>(void*, const uint8_t*, size_t, int, int, int, size_t, long long*);
extern template int points_load<2>(void*, const uint8_t*, size_t, int, int, int, size_t, long long*);
extern template int points_store<1>(uint8_t*, const void*, size_t, int, size_t);
extern template int points_store<2>(uint8_t*, const void*, size_t, int, size_t);
// point_diff.hip: out[i] = in[i + shift] - in[i], affine G1 records (the H bases of prepare_phase2); the same lane routine on the host
int g1_shifted_difference(void* d_out, const void* d_in, size_t n_in, size_t shift, size_t n_out, hipStream_t st);
int g1_shifted_difference_host(uint64_t* out, const uint64_t* in, size_t n_in, size_t shift, size_t n_out);
extern template int accumulator_transform<1>(uint8_t*, const uint8_t*, size_t, uint64_t, const uint64_t*, const uint64_t*, int, int, int, uint32_t, size_t, long long*);
extern template int accumulator_transform<2>(uint8_t*, const uint8_t*, size_t, uint64_t, const uint64_t*, const uint64_t*, int, int, int, uint32_t, size_t, long long*);
extern template int accumulator_power_pairs<1>(const uint8_t*, size_t, int, int, int, const uint32_t*, uint64_t, uint64_t, uint8_t*, size_t, uint64_t*, uint64_t*, long long*);
extern template int accumulator_power_pairs<2>(const uint8_t*, size_t, int, int, int, const uint32_t*, uint64_t, uint64_t, uint8_t*, size_t, uint64_t*, uint64_t*, long long*);
}  // namespace zk
