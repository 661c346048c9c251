#!/usr/bin/env python3
"""Local step after `gpurun -- bash tools/refresh_profiles.sh`: copies the summaries from gpurun_out/refresh/ into
profiles/ (round-tagged names) and rebuilds profiles/latest_pmc.json, which bench.py reports as roofline.traffic."""
import json, os, re, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpurun_out", "refresh"); DST = os.path.join(ROOT, "profiles")
tag = sys.argv[1] if len(sys.argv) > 1 else "r04_final"
def put(src, dst, header=None):
    body = open(os.path.join(SRC, src)).read()
    with open(os.path.join(DST, f"{tag}_{dst}"), "w") as f:
        if header: f.write(header)
        f.write(body)
put("bench_n1.json", "bench_n1.json"); put("bench_2e20.json", "bench_2e20.json"); put("g2_2e20.json", "g2_2e20.json")
put("next_rows_2e20.json", "next_rows_2e20.json"); put("ntt20.json", "ntt20.json")
put("contribute_2e20.json", "contribute_2e20.json"); put("host_entry.json", "host_entry.json"); put("shard_cells_2e26.json", "shard_cells_2e26.json")
put("ntt_16_20_24.json", "ntt_16_20_24.json"); put("skew_2e26.json", "skew_2e26.json"); put("bench_n1_tau.json", "bench_n1_tau.json")
put("table_mode.json", "table_mode.json"); put("ubench_valu.txt", "ubench_valu.txt"); put("ntt_other_sizes.json", "ntt_other_sizes.json"); put("ubench_fieldmul.txt", "ubench_fieldmul.txt"); put("ubench_wave_bucket.txt", "ubench_wave_bucket.txt"); put("prover.json", "prover.json"); put("skew_small.json", "skew_16_20.json")
put("msm26_kernel_stats.txt", "msm26_kernel_stats.txt",
    "# rocprofv3 --kernel-trace -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline   (MI355X, 2^26-point G1 MSM)\n"
    "# summarised from the rocpd database with tools/rocpd_summary.py (ROCm 7.2 rocprofv3 writes rocpd; same numbers as --stats)\n"
    "# batch_exp_kernel = synthetic-input generation (outside the timed region); every msm_* launch is a full-size step\n"
    "# (1 warm-up + 3 timed + 2 of the linearity check); msm_accumulate_kernel is the dominant kernel of a step\n")
put("ntt20_pass_sq_pmc.txt", "ntt20_pass_sq_pmc.txt", "# ntt_pass_wl_kernel<10> (round 5: the wave-local radix-4 pass), 2^20 elements (2 passes of 1024-point rows, 512 tiles of 2 x 1024, two 512-lane workgroups per CU), per dispatch,\n# rocprofv3 --pmc (two passes of 8 / 7 counters), tools/bench_ntt.py --log-n 20; SQ cycle counters tick once per 4 clocks\n")
put("msm20_timeline.txt", "msm20_timeline.txt", "# rocprofv3 --kernel-trace -- python tools/trace_one_msm.py: the launches of ONE 2^20-point G1 multiexp in order (start offset, duration incl. the\n# profiler's serialisation, gap to the previous kernel); the host join (~0.09 ms) follows the last copy\n")
put("ntt20_kernel_stats.txt", "ntt20_kernel_stats.txt", "# rocprofv3 --kernel-trace -- python tools/bench_ntt.py --check   (MI355X, 2^20 Fr NTT, 20 iterations x 4 ops)\n")
put("msm26_accumulate_sq_pmc.txt", "msm26_accumulate_sq_pmc.txt", "# rocprofv3 --pmc SQ_* (one pass, 8 counters) on msm_accumulate_kernel<Fq>, 2^26 points, MI355X\n")
with open(os.path.join(DST, f"{tag}_msm26_pmc_hbm.txt"), "w") as f:
    f.write("# rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline  (MI355X)\n"
            "# unit: KB per dispatch.  gfx950 FETCH_SIZE tallies 64 B per L2->fabric request: coalesced 16 B/lane streams (128-byte requests)\n"
            "# read half their bytes (msm_digits_hist_kernel: 2 GiB of scalars -> 1.05e6 KB), random 64-byte records and 16-byte words read\n"
            "# exactly 64 B per access (profiles/r02_ubench_gather_fetch_calibration.txt).  msm_accumulate_kernel is gathers only: no x2.\n")
    f.write(open(os.path.join(SRC, "msm26_pmc_fetch.txt")).read())
    f.write("".join(l for l in open(os.path.join(SRC, "msm26_pmc_write.txt")) if not l.startswith("kernel ")))
def counter(path, kernel):
    for l in open(os.path.join(SRC, path)):
        if l.startswith(kernel + " "): return float(l.split()[3])
    for l in open(os.path.join(SRC, path)):  # (template arguments beyond the field do not survive rocpd_summary's short())
        if l.startswith(kernel.split("<")[0]) and "<Fq>" in l: return float(l.split()[3])
    raise SystemExit(f"{kernel} not in {path}")
fetch = counter("msm26_pmc_fetch.txt", "zk::msm_accumulate_kernel<Fq>"); write = counter("msm26_pmc_write.txt", "zk::msm_accumulate_kernel<Fq>")
sys.path.insert(0, ROOT)
import bench
json.dump({"round": int(tag[1:3]), "workload_log_n": 26, "n_gpus": 1, "kernel": "msm_accumulate_kernel<Fq>", "FETCH_SIZE_KB_per_launch": fetch,
           "WRITE_SIZE_KB_per_launch": write, "hbm_bytes_per_launch": int((fetch + write) * 1024), "kernel_sources_sha": bench.kernel_sources_sha(),
           "how": f"rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes (profiles/{tag}_msm26_pmc_hbm.txt); bytes = (FETCH_SIZE + WRITE_SIZE)*1024: "
                  "the kernel reads through 64-byte base gathers and 16-byte index-list loads, which FETCH_SIZE tallies exactly (one 64-byte "
                  "request each, profiles/r02_ubench_gather_fetch_calibration.txt) -- the guide's x2 correction is for 128-byte streaming requests"},
          open(os.path.join(DST, "latest_pmc.json"), "w"), indent=1)
print(open(os.path.join(DST, "latest_pmc.json")).read())

# ---- the NTT pass's HBM counters, locked to ntt.hip + fieldu.hpp like the MSM figure is to its sources (round 5: bench.py carried a literal from round 3)
if os.path.exists(os.path.join(SRC, "ntt20_pmc_fetch.txt")):
    with open(os.path.join(DST, f"{tag}_ntt20_pmc_hbm.txt"), "w") as f:
        f.write("# rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) -- python tools/bench_ntt.py --log-n 20  (MI355X), KB per dispatch, averaged over\n"
                "# BOTH passes of the transforms (pass 1 also streams the 72-MiB table of inter-pass twiddles, pass 2 the 36-KiB root table).  The pass reads its data\n"
                "# as 16 B / lane coalesced streams: FETCH_SIZE tallies 64 B per 128-byte request there (the guide's x2); the table entries are read as 8-byte words of\n"
                "# consecutive lanes, the same streaming pattern.  Infinity-Cache hits are counted (32 MiB of data + the table fit its 256 MiB).\n")
        f.write(open(os.path.join(SRC, "ntt20_pmc_fetch.txt")).read())
        f.write("".join(l for l in open(os.path.join(SRC, "ntt20_pmc_write.txt")) if not l.startswith("kernel ")))
    nf = counter("ntt20_pmc_fetch.txt", "zk::ntt_pass_wl_kernel"); nw = counter("ntt20_pmc_write.txt", "zk::ntt_pass_wl_kernel")
    json.dump({"round": int(tag[1:3]), "workload_log_n": 20, "kernel": "ntt_pass_wl_kernel<10>", "FETCH_SIZE_KB_per_launch": nf, "WRITE_SIZE_KB_per_launch": nw,
               "hbm_bytes_per_launch": int((2 * nf + nw) * 1024), "kernel_sources_sha": bench.ntt_sources_sha(),
               "how": f"rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes over tools/bench_ntt.py --log-n 20 (profiles/{tag}_ntt20_pmc_hbm.txt), average of the "
                      "two passes of a transform; bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024: the reads are coalesced streams, which gfx950's FETCH_SIZE tallies at half "
                      "their bytes (guide); algorithmic 64 B x 2^20 = 67.1 MB per pass, the rest is the twiddle table of pass 1 (72 B per element)"},
              open(os.path.join(DST, "latest_pmc_ntt.json"), "w"), indent=1)
    print(open(os.path.join(DST, "latest_pmc_ntt.json")).read())

# ---- round 5 additions
for src, dst, hdr in (("ntt_pass_split.txt", "ntt_pass_split.txt", "# bash tools/ntt_pass_split.sh: rocprofv3 --kernel-trace over tools/bench_ntt.py --ops <op>, the pass launches by their position in the transform (last 40 transforms;\n# these run with the library's per-pass HIP events on: the gaps are longer than in the timed loop)\n"),
                      ("ntt_batch.json", "ntt_batch.json", None), ("ntt_streams.json", "ntt_streams.json", None),
                      ("ntt_no_fold.json", "ntt_no_fold.json", None)):
    if os.path.exists(os.path.join(SRC, src)): put(src, dst, hdr)

# ---- round 4 additions
for src, dst, hdr in (("ab_quad.txt", "ab_quad.txt", "# bash tools/ab_quad.sh: the reduce tails on quad additions (default) against one lane per addition (MI355ZK_MSM_QUAD=0), same box, same process order;\n# bench.py --log-n L --steps 30 --warmup 10 (ms per call, msm_reduce / msm_accumulate by HIP events, result limb) and tools/bench_g2.py\n"),
                      ("multi_device_2e26.json", "multi_device_2e26.json", None),
                      ("ntt_configs.txt", "ntt_configs.txt", "# bash tools/ab_ntt_lds.sh: tools/bench_ntt.py (warmed up, no per-pass events in the timed loop): (ms per transform, ntt_pass_kernel avg ms, passes)\n"),
                      ("ab_ntt_shoup.txt", "ab_ntt_shoup.txt", "# bash tools/ab_ntt_shoup.sh: the previous ntt.hip (Montgomery products by twiddles, libmi355zk_mont.so) against the products by a constant with its quotient, same box: (ms per transform, ntt_pass_kernel avg ms, passes)\n"),
                      ("host_entry_timeline.txt", "host_entry_timeline.txt", "# rocprofv3 --kernel-trace -- python tools/trace_host_entry.py: streamed host-buffer G1 multiexps at 2^26 over a pinned vector (page-locked exponents, 5 chunks), last 140 dispatches\n"),
                      ("ab_split.txt", "ab_split.txt", "# bash tools/ab_split.sh (ms per call; msm_accumulate / msm_reduce by HIP events; MI355ZK_MSM_SPLIT=0 = the lane-per-bucket launch alone)\n"),
                      ("bench_small.json", "bench_small.json", None),
                      ("msm16_timeline.txt", "msm16_timeline.txt", "# rocprofv3 --kernel-trace -- TRACE_LOG_N=16 python tools/trace_one_msm.py: the launches of ONE 2^16-point G1 multiexp\n")):
    if os.path.exists(os.path.join(SRC, src)): put(src, dst, hdr)

# ---- profiles/README.md is GENERATED from the files it describes (it drifted when it was written by hand: VERDICT r3 weak #10)
def J(name):
    try:
        txt = open(os.path.join(DST, f"{tag}_{name}")).read().strip()
        return json.loads(txt) if txt.startswith("{") and txt.count("\n{") == 0 else [json.loads(l) for l in txt.splitlines() if l.startswith("{")]
    except (OSError, ValueError):
        return None
def stat(kernel, path=f"{tag}_msm26_kernel_stats.txt", col=3):
    try:
        for l in open(os.path.join(DST, path)):
            if l.startswith(kernel + " "): return float(l.split()[col])
    except OSError:
        pass
    return None
rows = []
b = J("bench_n1.json")
if b:
    k = b["roofline"]["kernel_ms"]; sec = b.get("secondary", {}); h = b.get("incl_scalar_h2d") or {}
    rows.append((f"`{tag}_bench_n1.json`", "`python bench.py --full`", f"2^26 G1 MSM: `value` **{b['value']:.0f} Mscalar-mul/s** ({b['ms_per_step']:.2f} ms; HIP events: accumulate {k['msm_accumulate']:.2f}, digits {k['msm_digits']:.2f}, partition {k['msm_sort']:.2f}, reduce {k['msm_reduce']:.2f} ms); `value_incl_scalar_h2d` **{b['value_incl_scalar_h2d']:.0f}** ({h.get('ms_per_step')} ms; pageable {h.get('pageable_exponents_ms')}, page-locked {h.get('page_locked_exponents_ms')}, first call {h.get('first_call_incl_bases_h2d_ms')}); roofline frac {b['roofline']['frac']}; CPU: {b['cpu_baseline']['value']} M/s on {b['cpu_baseline']['cores']} threads"))
    n = sec.get("fr_ntt_2e20"); g1 = sec.get("g1_msm_2e20"); g2 = sec.get("g2_msm_2e20"); c = sec.get("contribute_2e20")
    if n and g1 and g2 and c:
        rows.append(("  `secondary`", "same run", f"2^20 Fr NTT fft / ifft / coset_fft {n['fft']['ms']} / {n['ifft']['ms']} / {n['coset_fft']['ms']} ms (pass {n['roofline']['pass_ms']} ms = {n['roofline']['achieved']} GB/s algorithmic); 2^20 G1 multiexp {g1['ms']} ms = {g1['value']} M/s (table mode {g1['table_mode']['ms']} ms = {g1['table_mode']['value']}); 2^20 G2 {g2['ms']} ms = {g2['value']} M/s (table mode {g2['table_mode']['ms']} = {g2['table_mode']['value']}); contribute 2^20 {c['ms']} ms = {c['value']} Mpoint/s"))
b20 = J("bench_2e20.json")
if b20: rows.append((f"`{tag}_bench_2e20.json`, `{tag}_msm20_timeline.txt`, `{tag}_msm16_timeline.txt`", "`bench.py --full --log-n 20 --no-secondary`; `rocprofv3 --kernel-trace -- tools/trace_one_msm.py`", f"BASELINE config 2: {b20['ms_per_step']} ms = {b20['value']:.0f} M/s (kernels: {b20['roofline']['kernel_ms']}); launch-by-launch timelines of one 2^20 and one 2^16 call"))
acc = stat("zk::msm_accumulate_kernel<Fq>")
if acc: rows.append((f"`{tag}_msm26_kernel_stats.txt`, `{tag}_msm26_pmc_hbm.txt`, `{tag}_msm26_accumulate_sq_pmc.txt`, `latest_pmc.json`", "`rocprofv3 --kernel-trace` / `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` / `--pmc SQ_*` (separate passes) `-- python bench.py ...`", f"`msm_accumulate_kernel<Fq>` avg **{acc / 1e3:.2f} ms** per launch; HBM traffic {(fetch + write) * 1024 / 1e9:.1f} GB per launch = {(fetch + write) * 1024 / (96 * 2**26):.1f} x the algorithmic 6.44 GB (FETCH {fetch * 1024 / 1e9:.1f} + WRITE {write * 1024 / 1e9:.1f})"))
nt = J("ntt_16_20_24.json")
if nt: rows.append((f"`{tag}_ntt20*.{{json,txt}}`, `{tag}_ntt_16_20_24.json`, `{tag}_ntt_other_sizes.json`, `{tag}_ntt_configs.txt`", "`tools/bench_ntt.py` (warm-up, no events in the timed loop), under `--kernel-trace` / `--pmc SQ_*`; `tools/ab_ntt_lds.sh`", "; ".join(f"2^{x['log_n']} fft {x['fft']['ms']} / ifft {x['ifft']['ms']} ms" for x in nt)))
he = J("host_entry.json")
if he: rows.append((f"`{tag}_host_entry.json`, `{tag}_host_entry_timeline.txt`", "`tools/bench_host_entry.py --log-n 20 24 26`; `rocprofv3 --kernel-trace -- tools/trace_host_entry.py`", "host-buffer entry point (streamed upload, pinned bases): " + json.dumps(he)[:600]))
sc = J("shard_cells_2e26.json")
if sc: rows.append((f"`{tag}_shard_cells_2e26.json`", "`tools/bench_shard_cells.py`", f"one rank's cell of an N-GPU run timed alone (single GPU {sc['one_gpu_ms']} ms): " + ", ".join(f"N={w}: {sc['n%d' % w]['cell_ms']} ms = {100 * sc['n%d' % w]['efficiency']:.0f} % of linear against that same-box time" for w in (2, 4, 8))))
md = J("multi_device_2e26.json")
if md: rows.append((f"`{tag}_multi_device_2e26.json`", "`tools/bench_multi_device.py`", f"single-process multi-GPU mode of the C ABI on {md['physical_gpus']} physical GPU(s) (repeated ids = logical devices sharing it: correctness / overhead, not scaling): " + ", ".join(f"{len(r['devices'])} cells {r['ms_per_call']} ms" for r in md["runs"])))
pr = J("prover.json")
if pr: rows.append((f"`{tag}_prover.json`", "`tools/bench_prover.py --log-m 16 / 20 / 22`", "; ".join(f"2^{x['log_m']}: sequential {x['sequential_ms']} ms, eight threads {x['eight_threads_ms']}, with tables {x['eight_threads_tables_ms']}" for x in pr)))
for name, cmd, what in (("ab_quad.txt", "`tools/ab_quad.sh`", "quad additions in the reduce tails against one lane per addition, same box (G1 2^12 .. 2^22, G2 2^12 .. 2^20)"),
                        ("ab_split.txt", "`tools/ab_split.sh`", "short calls: the long buckets on a quad each (msm_accumulate_split_kernel) against the lane-per-bucket launch alone, same box"),
                        ("bench_small.json", "`bench.py --log-n 12 / 14 / 16 / 20`", "the short calls after all of round 4's changes"),
                        ("table_mode.json", "`tools/bench_table.py`", "table mode against the plain call, same process"),
                        ("g2_2e20.json", "`tools/bench_g2.py`", "2^20 G2 multiexp with its closed-form check"),
                        ("next_rows_2e20.json", "`tools/bench_next_rows.py --log-n 20`", "SURVEY 8(f) rows 1-4 at 2^20"),
                        ("contribute_2e20.json", "`tools/bench_contribute.py`", "BASELINE config 5"),
                        ("skew_2e26.json", "`tools/bench_skew.py --log-n 26`", "prover-like exponents at 2^26"), ("skew_16_20.json", "`tools/bench_skew.py`", "prover-like exponents at 2^16 / 2^20"),
                        ("ubench_valu.txt", "`tools/bin/ubench_valu`", "issue cost of the VALU instructions the kernels are made of"),
                        ("ubench_fieldmul.txt", "`tools/bin/ubench_fieldmul`", "field product rates"), ("ubench_wave_bucket.txt", "`tools/bin/ubench_wave_bucket`", "lane per bucket vs wave per bucket"),
                        ("bench_n1_tau.json", "`python bench.py --full --bases tau`", "the headline on tau-table bases")):
    if os.path.exists(os.path.join(DST, f"{tag}_{name}")): rows.append((f"`{tag}_{name}`", cmd, what))
hand = [("`r04_exp_cu_mask.txt`", "`tools/exp_cu_mask.py`", "CU-masked side stream beside the accumulation: measured, rejected (DESIGN 6)"),
        ("`r04_small_n_sweep.txt`", "`tools/sweep_small_n.sh`", "every window width at 2^10 .. 2^20 and the reduce schedule after the quad additions: the measured table did not move"),
        ("`r04_reduce_schedule_sweep.txt`, `r04_partition_sweep.txt`", "`tools/sweep_reduce_schedule.sh`, `tools/sweep_partition.sh`", "forced reduce schedules (chunk lengths per level, hand-over to the trees) and partition geometries (super-tile size, fine bits) against the defaults: the defaults stay"),
        ("`r04_ntt20_isa_ledger.txt`", "`tools/ntt_isa_ledger.py [-DZK_NTT_LDS_PLANES]`", "static instruction ledger of `ntt_pass_kernel<10, radix-4>` by class, element-major LDS tiles against the limb planes of rounds 1-3 (84 vs 125 VGPRs)"),
        ("`r04_fuzz_msm.txt`", "`CASES=40 SEED=11 tools/fuzz_msm.sh`", "1240 differential fuzz cases against the oracle (window layouts, streamed chunks, table mode, 2 / 3 / 8 logical devices, one-lane tails): 0 mismatches"),
        ("`r04_ab_g1_pair.txt`, `r04_ab_g2_pair.txt`", "`tools/ab_g1_pair.sh`, `tools/ab_g2_pair.sh`", "the accumulation by a PAIR of lanes per bucket (`MI355ZK_G{1,2}_PAIR=1`) against one lane per bucket (`=0`) and the library's gate (auto), same box, 2^10 .. 2^22"),
        ("`r04_ab_g2_waves.txt`, `r04_ab_g2_waves_prover.txt`, `r04_ab_g2_small.txt`", "`tools/ab_g2_waves.sh`, `tools/ab_g2_waves_prover.sh`, `tools/ab_g2_small.sh`", "the one-lane G2 accumulation at two waves per SIMD against one: single calls 2^19 .. 2^24, and inside the prover's eight concurrent multiexps (why only a call that is alone takes two); the G2 short calls after the U-form doubling in the record additions"),
        ("`r04_small_n_sweep_pair.txt`", "`tools/sweep_small_n_pair.sh`", "every window width at 2^12 .. 2^18 with the pair kernels, G1 and G2: three table entries moved (G1 2^15, G2 2^15, G2 2^17)"),
        ("`r04_fuzz_msm_seed41.txt`", "`CASES=30 SEED=41 tools/fuzz_msm.sh`", "the differential fuzz on the final sources (every case of <= 3000 points now runs the pair kernels, plain and carried): 0 mismatches"),
        ("`r04_fuzz_msm_seed53.txt`", "`CASES=40 SEED=53 tools/fuzz_msm.sh` + seed 59 with `MI355ZK_G{1,2}_PAIR` forced", "1400 more differential cases on the final sources: 0 mismatches"),
        ("`r04_ab_split_pair.txt`", "`tools/ab_split.sh` on the final sources", "the quad-per-long-bucket launch on top of the pair kernels: still 1 - 4 % for G1 2^13 .. 2^15"),
        ("`r04_final_bench_n1_driver_style.json`", "`python bench.py` on a fresh box after the re-lock", "the line as the driver takes it: `roofline.traffic` filled from `latest_pmc.json` (same kernel sources), 1015 Mscalar-mul/s on that box"),
        ("`r04_host_entry_timeline.txt`, `r04_multi_device_2e26.json`", "mid-round copies of the files above", "kept: DESIGN cites them")]
hand5 = [("`r05_g2_exact_cost.json`", "`tools/bench_next_rows.py` (from `r05_final_next_rows_2e20.json`)", "the price of the exact G2 defaults on honest data: default vs `MI355ZK_G2_TRUSTED_SUBGROUP`, batch_exp 1.38-1.45 x, sparse matvec 1.14 / 1.78 x, point ifft 1.05 x"),
         ("`r05_table_mode_gc.txt`", "`python3 bench.py --gpus 1 --steps 20 --warmup 5` x 3, `tools/diag_table_calls.py`", "BENCH_r04's 3.24-ms G1 table-mode leg = one pause of the interpreter's cyclic GC inside 20 calls of 1.39 ms; per-call times, `host_gc`"),
         ("`r05_ubench_fieldmul.txt`", "`tools/bin/ubench_fieldmul`", "field products: memory format 125, U-form 167, f64 (5 x 52-bit, `v_fma_f64`, parity-checked) 110-117 G products/s = 0.66-0.70 x the U-form: not ported"),
         ("`r05_snop_ab.txt`", "`tools/build_nop_stripped.sh ntt msm_g1` + `tools/ab_snop.sh`", "the `s_nop 0` hipcc pads after every ZK_CHAIN_MAD pin, deleted from the assembly: accumulate 54.24 -> 53.83 ms, NTT 2^24 2.102 -> 2.090: < 1 %"),
         ("`r05_ntt_lds_model.txt`, `r05_ntt_lds_layout_ab.txt`", "`tools/ntt_lds_model.py`; `tools/ab_ntt_layout.sh`", "bank model of every LDS access site of the NTT pass (reproduces round 4's 20 % conflict cycles) and the measured counters: SQ_LDS_BANK_CONFLICT 884 736 -> 0; the pass time did not move"),
         ("`r05_ntt_warmup_ab.txt`", "`tools/bench_ntt.py --warm-ms 0 / 50`, `MI355ZK_NTT_WAVELOCAL=0 / 1`", "2^20 fft: barrier-per-pair kernel 0.124 / 0.1115 ms, wave-local kernel 0.1177 / 0.104 ms (5 ms / 50 ms of warm-up): the kernel change is 5-7 %, the rest was lukewarm clocks"),
         ("`r05_short_calls.txt`", "`tools/diag_short_calls.py`", "short multiexps: wall, kernel groups, host join before / after the branch-free host field arithmetic (G2 join 241 -> 184 us)"),
         ("`r05_multi_device_2e26.json`", "`tools/bench_multi_device.py --log-n 26 --devices 1 2 4 8`", "per-device cached base bytes = vector / N (slice residency), first call vs steady call, on one physical GPU"),
         ("`r05_heavy_past_reach.txt`", "`tests/test_gpu_msm.py::test_more_over_long_buckets_than_the_heavy_path_reaches` on the round-4 and round-5 libraries", "the dropped over-long bucket of ADVICE r4: wrong point before, right now"),
         ("`r05_fuzz_seed61.txt`", "`SEED=61 CASES=30 tools/fuzz_msm.sh`, `tools/fuzz_ntt.py --max-log 22`, `tools/fuzz_rows.py`", "1020 MSM + 150 NTT + 120 row-operation differential cases on the final sources: 0 mismatches"),
         ("`HISTORY_design_r1_r4.md`", "-", "DESIGN.md as it stood at the end of round 4 (the lab notebook of rounds 1-4)")]
with open(os.path.join(DST, "README.md"), "w") as f:
    f.write("# profiles/ — rocprofv3 evidence (MI355X, gfx950, ROCm 7.2)\n\n"
            "GENERATED by `tools/refresh_profiles_post.py` from the files it lists (after `gpurun -- bash tools/refresh_profiles.sh`): every number below is read\n"
            "from the file in the first column.  rocprofv3 in this image writes a rocpd SQLite database; the text files are per-kernel summaries made with\n"
            "`tools/rocpd_summary.py` / `tools/pmc_kernel.py`; PMC passes are separate runs, one counter group per pass (`/opt/skills/guides/MI355X_MICROARCH.md`).\n"
            "Rounds 1-3: `HISTORY.md`.\n\n| file | command | what it shows |\n|---|---|---|\n")
    for r in rows + hand5 + hand: f.write("| " + " | ".join(r) + " |\n")
print(open(os.path.join(DST, "README.md")).read()[:3000])
