// The device self-test ops (selftest_dev_ops.hpp) over fieldu.hpp as msm_g1.hip and ntt.hip build it: every column sum of a product one
// dependent chain of v_mad_u64_u32 (ZK_CHAIN_MAD, fieldu.hpp: u_mad).  The U-form ops over Fq and Fr and the G1 group law only.
#define ZK_CHAIN_MAD 1
#define ZK_ST_NS selftest_chain
#define ZK_ST_CHAIN 1
#include "selftest_dev_ops.hpp"

namespace zk {
int selftest_dev_launch_chain(int op, int which, const uint32_t* d_in, uint32_t* d_out, uint32_t blocks) {
  return selftest_chain::devop_launch(op, which, d_in, d_out, blocks);
}
}  // namespace zk
