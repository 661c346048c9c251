// G2 instantiation of the point FFT (point_fft_impl.hpp); see there for the design.
#include "point_fft_impl.hpp"

namespace zk {

int batch_normalize_g2(void* d_io_affine, const void* d_z, uint64_t n, hipStream_t st);   // scalar_mul.hip: 8 points per inversion

// d_points: 2^log_n affine raw G2 records (128 B), in place.  scale: every output is multiplied by scale_canon (ifft: m^-1).
int point_fft_g2(void* d_points, uint32_t log_n, const Fr& omega, bool scale, const Fr& scale_canon, hipStream_t st, bool trusted_subgroup) {
  return point_fft<G2U>(d_points, log_n, omega, scale, scale_canon, st, trusted_subgroup, batch_normalize_g2);
}

}  // namespace zk
