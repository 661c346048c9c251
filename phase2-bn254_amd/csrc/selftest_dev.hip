// mi355zk_selftest_dev_op (include/mi355zk.h): one field / group-law primitive per lane ON THE DEVICE, on operands chosen by the caller.
// Test infrastructure; the kernels are in selftest_dev_ops.hpp.  This unit builds them as msm_g2.hip, scalar_mul.hip and the point FFTs
// build fieldu.hpp (plain column sums); selftest_dev_chain.hip builds the ZK_CHAIN_MAD form (op | MI355ZK_DEVOP_CHAIN).
#define ZK_ST_NS selftest_plain
#define ZK_ST_CHAIN 0
#include "selftest_dev_ops.hpp"

#include "device_mem.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

namespace zk {
int selftest_dev_launch_chain(int op, int which, const uint32_t* d_in, uint32_t* d_out, uint32_t blocks);   // selftest_dev_chain.hip

namespace {
int selftest_dev_op(int op_flags, int which, const uint32_t* in, size_t in_words, uint32_t* out, size_t out_words, size_t n) {
  const bool chain = (op_flags & MI355ZK_DEVOP_CHAIN) != 0;
  const int op = op_flags & ~MI355ZK_DEVOP_CHAIN;
  if (op < 0 || op >= MI355ZK_DEVOP_END || (which != 0 && which != 1)) return ZK_ERR_BAD_ARGS;
  const selftest_plain::DevOpShape S = selftest_plain::devop_shape(op);
  if (S.in_words == 0 || in_words != (size_t)S.in_words || out_words != (size_t)S.out_words) return ZK_ERR_BAD_ARGS;
  if ((which == 1 && !S.fr) || (chain && !S.chain)) return ZK_ERR_BAD_ARGS;
  if (!in || !out || n == 0 || n % (size_t)S.group != 0 || n > ((size_t)1 << 22)) return ZK_ERR_BAD_ARGS;
  // whole workgroups: the last case again in the padding lanes (256 is a multiple of every group size, so the groups stay whole)
  const size_t n_pad = (n + 255) / 256 * 256;
  std::vector<uint32_t> h_in(n_pad * in_words);
  std::memcpy(h_in.data(), in, n * in_words * sizeof(uint32_t));
  for (size_t i = n; i < n_pad; ++i) std::memcpy(&h_in[i * in_words], &h_in[(i - S.group) * in_words], in_words * sizeof(uint32_t));   // (from h_in: already filled)
  std::vector<uint32_t> h_out(n_pad * out_words);
  // a test hook: plain allocations, the null stream and a device synchronise on the calling thread's CURRENT device -- not the library's
  // device set, pools or streams, which it neither uses nor disturbs
  DevTemp d_in, d_out;   // freed on every exit
  if (int rc = d_in.alloc(h_in.size() * sizeof(uint32_t))) return rc;
  if (int rc = d_out.alloc(h_out.size() * sizeof(uint32_t))) return rc;
  ZK_HIP(hipMemcpy(d_in.p, h_in.data(), h_in.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  ZK_HIP(hipMemset(d_out.p, 0xA5, h_out.size() * sizeof(uint32_t)));   // a result that is never written does not read as zero
  const uint32_t blocks = (uint32_t)(n_pad / 256);
  const int rc = chain ? selftest_dev_launch_chain(op, which, d_in.as<uint32_t>(), d_out.as<uint32_t>(), blocks)
                       : selftest_plain::devop_launch(op, which, d_in.as<uint32_t>(), d_out.as<uint32_t>(), blocks);
  if (rc != ZK_OK) return rc;
  ZK_HIP(hipDeviceSynchronize());
  ZK_HIP(hipMemcpy(h_out.data(), d_out.p, h_out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  // the padding lanes ran the last group again, so they must have written its results again: a padding lane that held anything else
  // (operands outside every contract, quads / pairs whose lanes disagree) is an error of this hook, not a result to discard
  for (size_t i = n; i < n_pad; ++i)
    if (std::memcmp(&h_out[i * out_words], &h_out[(i - S.group) * out_words], out_words * sizeof(uint32_t)) != 0) {
      fprintf(stderr, "mi355zk_selftest_dev_op: padding lane %zu did not repeat the last case (op %d)\n", i, op);
      return ZK_ERR_DEVICE;
    }
  std::memcpy(out, h_out.data(), n * out_words * sizeof(uint32_t));
  return ZK_OK;
}
}  // namespace
}  // namespace zk

extern "C" int mi355zk_selftest_dev_op(int op, int which, const uint32_t* in, size_t in_words_per_case, uint32_t* out, size_t out_words_per_case,
                                       size_t n_cases) {
  return zk::abi_guard([&]() -> int { return zk::selftest_dev_op(op, which, in, in_words_per_case, out, out_words_per_case, n_cases); });
}
