// G1 instantiation of the point FFT (point_fft_impl.hpp); see there for the design.
#include "point_fft_impl.hpp"

namespace zk {

int batch_normalize_g1(void* d_io_affine, const void* d_z, uint64_t n, hipStream_t st);   // scalar_mul.hip: 16 points per inversion

// d_points: 2^log_n affine raw records (64 B), in place.  scale: every output is multiplied by scale_canon (ifft: m^-1).
int point_fft_g1(void* d_points, uint32_t log_n, const Fr& omega, bool scale, const Fr& scale_canon, hipStream_t st) {
  return point_fft<G1U>(d_points, log_n, omega, scale, scale_canon, st, true, batch_normalize_g1);
}

}  // namespace zk
