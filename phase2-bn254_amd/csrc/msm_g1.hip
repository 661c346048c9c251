// G1 instantiation of the Pippenger pipeline (kernels: msm_impl.hpp, see there for the design; host driver: msm_host.hpp; the stages that
// do not depend on the group: msm_partition.hip).
#define ZK_CHAIN_MAD 1  // fieldu.hpp u_mad: one dependent mad chain per column (measured faster in this TU)
#include "msm_host.hpp"

namespace zk {

int msm_g1_device(const void* d_bases, uint64_t n_bases, uint64_t base_offset, const void* d_scalars, uint64_t n, const uint32_t* d_density,
                  const uint32_t* d_dprefix, hipStream_t st, uint64_t out_xyz[12], long long* err_index, uint32_t wgroups, uint32_t wgroup,
                  bool scalars_mont, MsmChunks* chunks, uint64_t table_stride, uint32_t table_c) {
  G1Jacobian r;
  int rc = msm_device<Fq>((const G1Affine*)d_bases, n_bases, base_offset, (const uint32_t*)d_scalars, n, d_density, d_dprefix, st, &r, err_index,
                          false, nullptr, nullptr, wgroups, wgroup, scalars_mont, chunks, table_stride, table_c);
  if (rc == ZK_OK) std::memcpy(out_xyz, &r, sizeof r);
  return rc;
}

// powersoftau::utils::dense_multiexp (powersoftau/src/utils.rs:189-292): bases.len() == exponents.len(), infinity
// bases add nothing; with d_bases2 the merge_pairs form (utils.rs:112-128, phase2/src/utils.rs:59-105): both
// base vectors against ONE exponent vector, sharing digit extraction and sorts.
int msm_g1_dense_device(const void* d_bases, const void* d_bases2, const void* d_scalars, uint64_t n, hipStream_t st, uint64_t* out_xyz,
                         uint64_t* out2_xyz) {
  G1Jacobian r, r2;
  long long err = -1;
  int rc = msm_device<Fq>((const G1Affine*)d_bases, n, 0, (const uint32_t*)d_scalars, n, nullptr, nullptr, st, &r, &err, true,
                          (const G1Affine*)d_bases2, d_bases2 ? &r2 : nullptr);
  if (rc == ZK_OK) {
    std::memcpy(out_xyz, &r, sizeof r);
    if (d_bases2 && out2_xyz) std::memcpy(out2_xyz, &r2, sizeof r2);
  }
  return rc;
}

// the dense call with the bucket tap of msm_host.hpp set: what the accumulate stage left, for mi355zk_selftest_g1_msm_buckets_dev
int msm_g1_buckets_device(const void* d_bases, const void* d_scalars, uint64_t n, hipStream_t st, uint64_t out_xyz[12], uint32_t* n_buckets, uint32_t* n_vals,
                          uint32_t* first, uint32_t* last, size_t cap_buckets, uint32_t* vals, size_t cap_vals, uint64_t* records) {
  MsmBucketTap tap;
  g_msm_bucket_tap = &tap;
  const int rc = msm_g1_dense_device(d_bases, nullptr, d_scalars, n, st, out_xyz, nullptr);
  g_msm_bucket_tap = nullptr;
  if (rc != ZK_OK) return rc;
  *n_buckets = tap.n_buckets;
  *n_vals = (uint32_t)tap.vals.size();
  if (tap.n_buckets > cap_buckets || tap.vals.size() > cap_vals) return ZK_ERR_BAD_ARGS;   // (the two counts tell the caller what to bring)
  std::memcpy(first, tap.first.data(), tap.first.size() * 4);
  std::memcpy(last, tap.last.data(), tap.last.size() * 4);
  if (!tap.vals.empty()) std::memcpy(vals, tap.vals.data(), tap.vals.size() * 4);
  std::memcpy(records, tap.records.data(), tap.records.size() * 8);
  return ZK_OK;
}

int segsum_g1_device(const void* d_points, uint64_t nnz, const uint32_t* d_row_ptr, uint32_t n_rows, hipStream_t st, void* d_out) {
  return segsum_device<Fq>((const G1Affine*)d_points, nnz, d_row_ptr, n_rows, st, (G1Affine*)d_out);
}

// a batch of exponent vectors over one base vector (msm_host.hpp: msm_device_batch): out_xyz = n_vectors x 12 words
int msm_g1_batch_device(const void* d_bases, uint64_t n_bases, uint64_t base_offset, const void* d_scalars, uint64_t n, uint64_t scalar_stride,
                        uint32_t n_vectors, const uint32_t* d_density, const uint32_t* d_dprefix, hipStream_t st, uint64_t* out_xyz, int* rcs,
                        long long* err_indices, bool scalars_mont) {
  std::vector<G1Jacobian> r(n_vectors);
  int rc = msm_device_batch<Fq>((const G1Affine*)d_bases, n_bases, base_offset, (const uint32_t*)d_scalars, n, scalar_stride, n_vectors, d_density, d_dprefix, st,
                                r.data(), rcs, err_indices, scalars_mont);
  if (rc == ZK_OK)
    for (uint32_t v = 0; v < n_vectors; ++v)
      if (rcs[v] == ZK_OK) std::memcpy(out_xyz + (size_t)v * 12, &r[v], sizeof r[v]);
  return rc;
}

void msm_release_g1() { ws_release_all(); }

}  // namespace zk
