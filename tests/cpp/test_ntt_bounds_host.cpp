// Bound checker for the Fr transform's lazy butterfly chain: the lines of csrc/ntt_butterfly.hpp -- the butterfly, the load- and store-side
// products, the closing reductions, the scale kernel's and the table builders' element lines -- INSTANTIATED on limbs that carry worst-case
// intervals (tests/cpp/u_interval.hpp; read its head for what is tracked).  Host compiler only; tests/test_ntt_bounds_host.py builds and runs it.
//   test_ntt_bounds_host                 an INDUCTION over the stages.  The checker is given one thing, the load state "canonical: < p, N-form";
//                                        every later state is derived: stage s is ntt_bf<s> applied to (u, t), both anywhere in the state
//                                        before it, once per skip flag the kernels' own rule can produce there, and the union of all outputs
//                                        is the state before stage s + 1.  For every row length 2^1 .. 2^12, for the radix-2 rule, the
//                                        radix-4 / wave-local rule and the twisted path (no skip; a product at stage 0), from the state after
//                                        every load mode, into every store mode; then the straight-line cases.  Every (kernel kind, LOG_NP,
//                                        pre, post, twiddle mode) the planner (csrc/ntt_plan.hpp) can emit, over log_n 1 .. 30, the four
//                                        domain operations and the knobs, must be among the chains run.  Prints the value bound and the
//                                        largest limb after every stage; exit 0 only with no violation.
//   test_ntt_bounds_host bite_skip3      schedule with skip_max = 3 at LOG_NP = 10: must report u_sub's value precondition or u_to_std_lt32p's
//   test_ntt_bounds_host bite_carry8     sums carried every 8th stage: must report u_mul_shoup's limb precondition or a wrapping limb
//   test_ntt_bounds_host bite_sub2       the skipped stage-2 subtraction done with u_sub<2, 1>: must report value(b) not within K p
//   test_ntt_bounds_host bite_unhooked   an element no hook has bounded is fed to u_to_std_lt2p: must be reported, not passed
// (each bite mode exits 0 only if the named report appears)
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <tuple>

#include "u_interval.hpp"

#include "../../phase2-bn254_amd/csrc/ntt_butterfly.hpp"
#include "../../phase2-bn254_amd/csrc/ntt_plan.hpp"

using namespace zk;
using PRM = FrParams;
using F = FrU;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 3;
}
static const char* keep(const std::string& s) {
  static std::deque<std::string> names;
  names.push_back(s);
  return names.back().c_str();
}

// a concrete canonical element in the memory format (the top word below the modulus's)
static Fr some_canonical_words() {
  Fr c;
  for (int i = 0; i < 7; ++i) c.l[i] = rnd() * 8u + (rnd() & 7u);
  c.l[7] = rnd() % PRM::P[7];
  return c;
}
// THE load state: what ntt_load returns (its hook says: canonical), with the limbs widened to anywhere a canonical N-form element can be
static F load_state() {
  F r = ntt_load(some_canonical_words());
  for (int i = 0; i < 8; ++i) r.l[i] = IvLimb(r.l[i].v, 0, U_MASK);
  r.l[8] = IvLimb(r.l[8].v, 0, UParams<PRM>::P(8));
  return r;
}
// any table constant: a consistent concrete pair (w, wq) rides along, the intervals are those of every canonical w and its quotient
static TwU any_twiddle() {
  TwU t = tw_make(some_canonical_words());
  for (int i = 0; i < 8; ++i) t.w.l[i] = IvLimb(t.w.l[i].v, 0, U_MASK);
  t.w.l[8] = IvLimb(t.w.l[8].v, 0, UParams<PRM>::P(8));
  for (int i = 0; i < 9; ++i) t.q.l[i] = IvLimb(t.q.l[i].v, 0, U_MASK);
  return t;
}
static const auto lazy_twiddle = [] { return any_twiddle(); };

static double limb_multiple(const F& a) {   // the largest of limbs 0..7, in units of 2^29
  int64_t m = 0;
  for (int i = 0; i < 8; ++i)
    if (a.l[i].hi > m) m = a.l[i].hi;
  return (double)(m + 1) / 536870912.0;
}
static void unite(F& acc, const F& x, bool first) {
  if (first) acc = x;
  else UChk::either(acc, acc, x);
}

enum Pattern { PAT_R2 = 0, PAT_R4 = 1, PAT_TWISTED = 2 };   // the radix-2 loop's rule; the radix-4 and wave-local kernels' rule; pre >= 3
static const char* const pattern_name[3] = {"plain, radix-2 rule", "plain, radix-4 / wave-local rule", "twisted (no skip)"};

// the skip flags the kernels' own rules can produce at stage s of a row of 2^LOG_NP (ntt.hip: `skip` of the radix-2 loop, `one` / `one2`
// of the radix-4 kernels, `!twisted` of the lone stage 0)
template <uint32_t LOG_NP, class SCH>
static void skip_flags(Pattern pat, uint32_t s, bool& can_skip, bool& can_multiply) {
  constexpr uint32_t np = 1u << LOG_NP;
  if (pat == PAT_TWISTED) { can_skip = false; can_multiply = true; return; }
  if (s == 0) { can_skip = true; can_multiply = false; return; }              // stage 0: every twiddle is one
  if (pat == PAT_R2) {
    const bool j_slow = SCH::may_skip(s) && (np >> (s + 1)) >= 64;            // twiddle index uniform over a wave: j == 0 skips
    can_skip = j_slow; can_multiply = true; return;
  }
  can_skip = SCH::may_skip(s); can_multiply = true;                           // a lane whose j is 0 skips
}

// the stages of one row: returns the state after the last one
template <uint32_t LOG_NP, class SCH>
static F chain(Pattern pat, const F& start, bool print) {
  F state = start;
  if (print) std::printf("    load      value < %6.3f p   limbs < %5.2f * 2^29\n", state.vb, limb_multiple(state));
  for_limbs<(int)LOG_NP>([&](auto sc) {
    constexpr uint32_t s = (uint32_t) decltype(sc)::value;
    bool can_skip = false, can_multiply = false;
    skip_flags<LOG_NP, SCH>(pat, s, can_skip, can_multiply);
    F next;
    bool first = true;
    for (int flag = 0; flag < 2; ++flag) {
      const bool skip = flag != 0;
      if (skip ? !can_skip : !can_multiply) continue;
      F u = state, t = state;                                                 // both anywhere in the current state
      if (pat == PAT_R2) {
        F sum, dif;
        ntt_bf_to<s, SCH>(u, t, lazy_twiddle, skip, sum, dif);
        unite(next, sum, first), unite(next, dif, false);
      } else {
        ntt_bf<s, SCH>(u, t, any_twiddle(), skip);
        unite(next, u, first), unite(next, t, false);
      }
      first = false;
    }
    state = next;
    if (print)
      std::printf("    stage %-2u%s value < %6.3f p   limbs < %5.2f * 2^29%s\n", s, (LOG_NP & 1) && s == 0 && pat != PAT_R2 ? "*" : " ", state.vb, limb_multiple(state),
                  can_skip ? (can_multiply ? "   (skipped or multiplied)" : "   (skipped)") : "");
  });
  return state;
}

// the state after a load mode
static F after_pre(uint32_t pre) {
  F v = load_state();
  if (pre == 1) v = ntt_pre1(v, any_twiddle(), lazy_twiddle);
  else if (pre == 2) v = ntt_pre2(v, any_twiddle());
  else if (pre == 4) v = ntt_pre4(v, any_twiddle());
  return v;                                                                   // pre == 0, 3: no product at the load
}

// store modes: what the pass kernels' store code does with the last stage's state, by (tw_full, tw_mul != 0, post)
enum StoreMode { ST_TW_FULL = 0, ST_TW_TWO = 1, ST_POST1 = 2, ST_POST2 = 3, ST_POST3 = 4, ST_POST4 = 5, ST_POST5 = 6, ST_MODES = 7 };
static const char* const store_name[ST_MODES] = {"full-table twiddle", "two-level twiddle", "post 1 (post_c)", "post 2 (A * B * post_c)", "post 3 (u_to_std_lt32p)",
                                                 "post 4 (row table)", "post 5 (row constant * row table)"};
static void store(StoreMode m, const F& last) {
  F v = last;
  switch (m) {
    case ST_TW_FULL: (void)ntt_store_mul(v, any_twiddle()); break;
    case ST_TW_TWO: v = ntt_post_mul(v, any_twiddle()); (void)ntt_store_mul(v, any_twiddle()); break;
    case ST_POST1: (void)ntt_store_mul(v, any_twiddle()); break;
    case ST_POST2: v = ntt_post_mul2(v, any_twiddle(), lazy_twiddle); (void)ntt_store_mul(v, any_twiddle()); break;
    case ST_POST3: (void)ntt_store_plain(v); break;
    case ST_POST4: (void)ntt_store_mul(v, any_twiddle()); break;
    case ST_POST5: v = ntt_post_mul(v, any_twiddle()); (void)ntt_store_mul(v, any_twiddle()); break;
    default: break;
  }
  // (the barrier kernels close with ntt_post_mul and ntt_reduce_lt2p, the wave-local one with ntt_store_mul: the same two lines)
  F w = ntt_post_mul(last, any_twiddle());
  (void)ntt_reduce_lt2p(w);
}
static StoreMode store_mode_of(const NttPassParams& P) {
  if (P.tw_full) return ST_TW_FULL;
  if (P.tw_mul != 0) return ST_TW_TWO;
  switch (P.post) {
    case 2: return ST_POST2;
    case 3: return ST_POST3;
    case 4: return ST_POST4;
    case 5: return ST_POST5;
    default: return ST_POST1;
  }
}

using Combo = std::tuple<uint32_t, uint32_t, uint32_t, int>;   // pattern, LOG_NP, pre, store mode

template <template <uint32_t> class SCHT>
static void run_rows(std::set<Combo>* ran, uint32_t only_log_np, bool print) {
  for_limbs<NTT_MAX_LOG_NP>([&](auto lc) {
    constexpr uint32_t LOG_NP = (uint32_t) decltype(lc)::value + 1;
    if (only_log_np && LOG_NP != only_log_np) return;
    using SCH = SCHT<LOG_NP>;
    for (int pat = 0; pat < 3; ++pat)
      for (uint32_t pre = 0; pre <= 4; ++pre) {
        if ((pat == PAT_TWISTED) != (pre >= 3)) continue;                     // pre 3 / 4 are the twisted path, and only they
        u_violations().where = keep("rows of 2^" + std::to_string(LOG_NP) + ", " + pattern_name[pat] + ", pre " + std::to_string(pre));
        if (print) std::printf("  %s   (skip_max %u)\n", u_violations().where, SCH::skip_max);
        const F last = chain<LOG_NP, SCH>((Pattern)pat, after_pre(pre), print);
        for (int m = 0; m < ST_MODES; ++m) {
          if (m == ST_POST5 && pat != PAT_TWISTED && pat != PAT_R4) continue;  // the wave-local kernel's alone
          u_violations().where = keep("rows of 2^" + std::to_string(LOG_NP) + ", " + pattern_name[pat] + ", pre " + std::to_string(pre) + ", store: " + store_name[m]);
          store((StoreMode)m, last);
          if (ran) ran->insert(Combo{(uint32_t)pat, LOG_NP, pre, m});
        }
      }
  });
}

// every (kernel kind, LOG_NP, pre, store mode) the planner can emit must be among the chains that ran
static size_t check_planner_combinations(const std::set<Combo>& ran) {
  std::set<std::tuple<uint32_t, uint32_t, uint32_t, int>> seen;   // kind, LOG_NP, pre, store mode
  const int lognps[4] = {0, 10, 11, 12}, tiles[4] = {0, 1024, 2048, 4096}, radices[3] = {0, 2, 4};
  u_violations().where = "planner";
  for (uint32_t log_n = 1; log_n <= 30; ++log_n)
    for (int op = 0; op < 4; ++op)
      for (int lg : lognps)
        for (int tl : tiles)
          for (int rx : radices)
            for (int bits = 0; bits < 16; ++bits) {
              NttKnobs K;
              K.lognp = lg, K.tile = tl, K.radix = rx;
              K.no_wavelocal = bits & 1, K.no_full_tw = (bits & 2) != 0, K.no_fold = (bits & 4) != 0, K.no_stage_fold = (bits & 8) != 0;
              NttRequest Q;
              Q.log_n = log_n;
              Q.pre_g = op == 2;                       // fft, ifft, coset_fft, icoset_fft (api: which factors each passes)
              Q.post_c = op == 1 || op == 3;
              Q.post_g = op == 3;
              NttPlan N;
              if (ntt_plan(Q, K, &N) != ZK_OK) continue;   // a refused request launches nothing
              for (int p = 0; p < N.R; ++p) {
                const NttPass& pass = N.pass[p];
                const int mode = store_mode_of(pass.P);
                if (!seen.insert({(uint32_t)pass.kind, pass.P.log_np, pass.P.pre, mode}).second) continue;
                if (pass.kind != NTT_KERNEL_WL && (pass.P.pre > 2 || pass.P.post > 4))
                  u_violations().add("the planner gives a barrier kernel pre " + std::to_string(pass.P.pre) + " / post " + std::to_string(pass.P.post) + ", which it does not know");
                const uint32_t pat = pass.P.pre >= 3 ? PAT_TWISTED : pass.kind == NTT_KERNEL_R2 ? PAT_R2 : PAT_R4;
                if (!ran.count(Combo{pat, pass.P.log_np, pass.P.pre, mode}))
                  u_violations().add("no chain was run for kind " + std::to_string(pass.kind) + ", rows of 2^" + std::to_string(pass.P.log_np) + ", pre " +
                                     std::to_string(pass.P.pre) + ", store: " + store_name[mode]);
              }
            }
  return seen.size();
}

// ntt_scale_kernel's line and the two full-table builders', as straight-line cases
static void run_straight_lines() {
  Fr c;   // the largest canonical constant: p - 1
  for (int i = 0; i < 8; ++i) c.l[i] = PRM::P[i];
  c.l[0] -= 1;
  u_violations().where = "ntt_scale_kernel (a *= c)";
  F v = ntt_scale_const(load_state(), c);
  std::printf("  %-52s value < %6.3f p\n", u_violations().where, v.vb);
  (void)ntt_reduce_lt2p(v);
  u_violations().where = "ntt_scale_kernel (a *= c * A * B)";
  v = ntt_scale_pow(ntt_scale_const(load_state(), c), any_twiddle(), lazy_twiddle);
  std::printf("  %-52s value < %6.3f p\n", u_violations().where, v.vb);
  (void)ntt_reduce_lt2p(v);
  u_violations().where = "ntt_full_twiddle_kernel";
  F w = ntt_tab_product(any_twiddle(), any_twiddle());
  std::printf("  %-52s value < %6.3f p\n", u_violations().where, w.vb);
  (void)ntt_tab_entry(w);
  u_violations().where = "ntt_full_folded_kernel";
  w = ntt_tab_product(any_twiddle(), any_twiddle());
  w = ntt_tab_factor2(w, any_twiddle(), lazy_twiddle);
  w = ntt_tab_factor2(w, any_twiddle(), lazy_twiddle);
  w = ntt_tab_factor(w, any_twiddle());
  std::printf("  %-52s value < %6.3f p\n", u_violations().where, w.vb);
  (void)ntt_tab_entry(w);
}

static int run_all() {
  std::set<Combo> ran;
  run_rows<NttSchedule>(&ran, 0, true);
  run_straight_lines();
  const size_t planned = check_planner_combinations(ran);
  std::printf("%zu chains into store modes run; %zu distinct (kernel kind, LOG_NP, pre, store mode) combinations planned, all among them\n", ran.size(), planned);
  for (const auto& s : u_violations().list) std::printf("VIOLATION %s\n", s.c_str());
  std::printf("%zu violations\n", u_violations().list.size());
  return u_violations().list.empty() ? 0 : 1;
}

// ---- broken schedules: the checker must say so ----
template <uint32_t LOG_NP>
struct SchSkip3 : NttSchedule<LOG_NP> {   // stage 3 skipped too (with the subtraction constant that would go with it)
  static constexpr uint32_t skip_max = 3;
  static constexpr bool may_skip(uint32_t st) { return st <= skip_max; }
  static constexpr int skip_sub_k(uint32_t st) { return (st >= 1 && st <= skip_max) ? (2 << st) : 2; }
};
template <uint32_t LOG_NP>
struct SchCarry8 : NttSchedule<LOG_NP> {  // sums carried every 8th stage
  static constexpr bool carry_sum(uint32_t st) { return (st & 7) == 7; }
};
template <uint32_t LOG_NP>
struct SchSub2 : NttSchedule<LOG_NP> {    // the skipped stage-2 subtraction with K = 2
  static constexpr int skip_sub_k(uint32_t st) { return st == 1 ? 4 : 2; }
};

static int reported(const std::vector<const char*>& any_of) {
  bool said = false;
  for (const auto& s : u_violations().list) {
    std::printf("REPORTED %s\n", s.c_str());
    for (const char* what : any_of)
      if (s.find(what) != std::string::npos) said = true;
  }
  std::printf("%s\n", said ? "the required report appeared" : "the required report is MISSING");
  return said ? 0 : 1;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "bite_skip3")) {
    run_rows<SchSkip3>(nullptr, 10, false);
    return reported({"> precondition: value(b)", "u_to_std_lt32p precondition: value"});
  }
  if (!std::strcmp(mode, "bite_carry8")) {
    run_rows<SchCarry8>(nullptr, 0, false);
    return reported({"u_mul_shoup precondition: limb", "limb expression can wrap"});
  }
  if (!std::strcmp(mode, "bite_sub2")) {
    run_rows<SchSub2>(nullptr, 0, false);
    return reported({", 1> precondition: value(b)"});
  }
  if (!std::strcmp(mode, "bite_unhooked")) {
    u_violations().where = "an element no hook has bounded";
    F x;                                        // limbs of a small number; no function with a result hook made it
    for (int i = 0; i < 9; ++i) x.l[i] = IvLimb(i == 0 ? 5u : 0u);
    (void)ntt_reduce_lt2p(x);
    return reported({"u_to_std_lt2p precondition: value"});
  }
  if (mode[0]) {
    std::fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  return run_all();
}
