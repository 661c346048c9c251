#!/usr/bin/env python3
"""Ceremony verification on one MI355X -> profiles/ceremony_verify.md.

Without --section this is the driver: it runs each section below as a child process of its own under a time limit (--limit seconds each),
stops at the first child that fails or runs out of time, and writes the rows the children printed (one JSON line each) as a table.

  fill      mi355zk_bn254_fr_random_dev at 2^20 and 2^24 scalars: ms, GB/s written
  merge     merge_pairs_random_dev against merge_pairs_dev with resident rho, G1 and G2 at 2^20: the expectation is the fill on top
  host      host-buffer merge_pairs_random against host-buffer merge_pairs with rho drawn by numpy and uploaded, G1 at 2^22, both timed
            with the draw included: the claim the entry point rests on
  phase2    verify_contribution at |H| = |L| = 2^20: decode, multiexps, subgroup check, the one pairing launch, total
  tau       verify_transform at power 16, the same split

Times are medians of --iters calls after --warm calls, each to a synchronised device."""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SECTIONS = ("fill", "merge", "host", "phase2", "tau")
ap = argparse.ArgumentParser()
ap.add_argument("--section", choices=SECTIONS); ap.add_argument("--iters", type=int, default=5); ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--limit", type=int, default=150); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ceremony_verify.md"))
ap.add_argument("--log-h", type=int, default=20); ap.add_argument("--power", type=int, default=16)
a = ap.parse_args()


def driver():
    rows, note = [], None
    for sec in SECTIONS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--section", sec, "--iters", str(a.iters), "--warm", str(a.warm),
               "--log-h", str(a.log_h), "--power", str(a.power)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                rows.append(json.loads(ln)); print(ln, flush=True)
        if r.returncode != 0:
            note = f"section `{sec}` ended with status {r.returncode}; the sections after it were not run"
            print(note, r.stderr[-2000:], file=sys.stderr, flush=True)
            break
    with open(a.out, "w") as f:
        f.write("# Ceremony verification: measurements\n\nWritten by `tools/bench_ceremony_verify.py` (medians of %d calls after %d warm-up calls, device synchronised; "
                "one child process per section).\n\n| section | what | ms | detail |\n|---|---|---|---|\n" % (a.iters, a.warm))
        for row in rows:
            detail = ", ".join(f"{k} = {v}" for k, v in row.items() if k not in ("section", "what", "ms"))
            f.write(f"| {row['section']} | {row['what']} | {row.get('ms', '')} | {detail} |\n")
        if note:
            f.write(f"\n{note}\n")
    return 1 if note else 0


if a.section is None:
    sys.exit(driver())

import numpy as np, torch  # noqa: E402
import phase2_bn254_amd as zk, inputs  # noqa: E402
L = zk.lib.load(); zk.Worker(0)
KEY = bytes(range(32))


def timed(fn):
    for _ in range(a.warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 3)


def emit(what, ms=None, **kw):
    print(json.dumps({"section": a.section, "what": what, "ms": ms, **kw}), flush=True)


def points(group, n, seed):
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
    k = zk.ceremony.fr_random(n, KEY, 1000 + seed)
    p = torch.empty((n, 8 * group), dtype=torch.int64, device="cuda")
    fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
    assert fn(C.c_void_p(p.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0
    torch.cuda.synchronize()
    return p


class Split:
    """wall time, device synchronised, spent inside some functions of the flows during one call"""

    def __init__(self, targets):
        self.targets, self.ms, self.saved = targets, {}, []

    def __enter__(self):
        for label, (mod, name) in self.targets.items():
            real = getattr(mod, name)
            self.saved.append((mod, name, real))

            def wrapped(*args, _real=real, _label=label, **kw):
                torch.cuda.synchronize(); t = time.perf_counter()
                out = _real(*args, **kw)
                torch.cuda.synchronize(); self.ms[_label] = self.ms.get(_label, 0.0) + (time.perf_counter() - t) * 1e3
                return out

            setattr(mod, name, wrapped)
        return self

    def __exit__(self, *exc):
        for mod, name, real in self.saved: setattr(mod, name, real)


FLOW_TARGETS = {"multiexps_ms": (zk.ceremony, "merge_pairs_random"), "subgroup_check_ms": (zk.ceremony, "g2_subgroup_check"),
                "pairing_launch_ms": (zk.pairing, "same_ratio_batch"), "hash_to_g2_ms": (zk.keys, "hash_to_g2")}

if a.section == "fill":
    for lg in (20, 24):
        n = 1 << lg
        out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        key = zk.ceremony._chacha_key(KEY)
        ms = timed(lambda: L.mi355zk_bn254_fr_random_dev(out.data_ptr(), n, key, 1, 0, None))
        ok = bool(np.array_equal(out[-3:].cpu().numpy().view(np.uint64), zk.ceremony.fr_random_host(3, KEY, 1, n - 3)))
        emit(f"fr_random_dev 2^{lg}", ms, GB_per_s=round(n * 32 / ms / 1e6, 1), matches_host=ok)
elif a.section == "merge":
    n = 1 << 20
    for group in (1, 2):
        v = points(group, n + 1, group)
        rho = zk.ceremony.fr_random(n, KEY, 5)
        base = timed(lambda: zk.ceremony.merge_pairs(v[:n], v[1:], rho))
        rnd = timed(lambda: zk.ceremony.merge_pairs_random(v[:n], v[1:], KEY, 5))
        same = bool(np.array_equal(zk.prover._to_affine(zk.ceremony.merge_pairs(v[:n], v[1:], rho)[0]), zk.prover._to_affine(zk.ceremony.merge_pairs_random(v[:n], v[1:], KEY, 5)[0])))
        emit(f"G{group} merge_pairs_dev 2^20, resident rho", base)
        emit(f"G{group} merge_pairs_random_dev 2^20", rnd, difference_ms=round(rnd - base, 3), same_point=same)
elif a.section == "host":
    n = 1 << 22
    v = np.ascontiguousarray(points(1, n + 1, 7).cpu().numpy().view(np.uint64))
    rng = np.random.default_rng(1)

    def with_numpy():
        rho = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        rho[:, 3] &= np.uint64((1 << 61) - 1)
        return zk.ceremony.merge_pairs_host(v[:n], v[1:], rho)

    base = timed(with_numpy)
    rnd = timed(lambda: zk.ceremony.merge_pairs_random_host(v[:n], v[1:], KEY, 5))
    draw = timed(lambda: rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64))
    emit("host merge_pairs G1 2^22, rho drawn by numpy and uploaded", base, numpy_draw_alone_ms=draw)
    emit("host merge_pairs_random G1 2^22", rnd, difference_ms=round(rnd - base, 3))
elif a.section == "phase2":
    n = 1 << a.log_h
    dev = torch.device("cuda", 0)
    one1 = torch.from_numpy(zk.ceremony.G1_ONE_RAW.view(np.int64).reshape(1, 8)).to(dev)
    one2 = torch.from_numpy(zk.ceremony.G2_ONE_RAW.view(np.int64).reshape(1, 16)).to(dev)
    small1, small2 = points(1, 4, 31), points(2, 4, 32)
    vk = {"alpha_g1": small1[:1], "beta_g1": small1[1:2], "beta_g2": small2[:1], "gamma_g2": one2, "delta_g1": one1, "delta_g2": one2, "ic": small1[2:4].contiguous()}
    params = {"vk": vk, "h": points(1, n, 33), "l": points(1, n, 34), "a": small1, "b_g1": small1, "b_g2": small2}
    mpc0 = {"params": params, "cs_hash": torch.zeros(64, dtype=torch.uint8, device=dev), "contributions": []}
    mpc1, _ = zk.contribute_mpc_parameters(mpc0)
    t_contrib = timed(lambda: zk.contribute_mpc_parameters(mpc1))
    mpc2, h2 = zk.contribute_mpc_parameters(mpc1)
    blob = zk.ceremony.write_mpc_parameters(mpc2)
    t_decode = timed(lambda: zk.ceremony.read_mpc_parameters(blob))
    assert zk.verify_contribution(mpc1, mpc2) == h2
    total = timed(lambda: zk.verify_contribution(mpc1, mpc2))
    with Split(FLOW_TARGETS) as sp:
        zk.verify_contribution(mpc1, mpc2)
    emit(f"contribute_mpc_parameters |H| = |L| = 2^{a.log_h}", t_contrib)
    emit(f"read_mpc_parameters (decode, checked) of the {blob.numel() >> 20} MiB file", t_decode)
    emit(f"verify_contribution |H| = |L| = 2^{a.log_h}", total, **{k: round(v, 3) for k, v in sp.ms.items()})
elif a.section == "tau":
    dev = torch.device("cuda", 0)
    FLOW_TARGETS["multiexps_ms"] = (zk.ceremony, "power_pairs_random")
    challenge = zk.ceremony.write_accumulator(zk.ceremony.new_accumulator(a.power, dev), compressed=False)
    t_contrib = timed(lambda: zk.contribute_response(challenge, a.power))
    response, _ = zk.contribute_response(challenge, a.power)
    digest = zk.ceremony.calculate_hash(challenge)
    t_decode = timed(lambda: zk.verify.read_response(response, a.power))
    before = zk.ceremony.read_accumulator(challenge, a.power, compressed=False)
    after, pub = zk.verify.read_response(response, a.power)
    assert zk.verify_transform(before, after, pub, digest)
    total = timed(lambda: zk.verify_transform(before, after, pub, digest))
    with Split(FLOW_TARGETS) as sp:
        zk.verify_transform(before, after, pub, digest)
    emit(f"contribute_response power {a.power}", t_contrib)
    emit(f"read_response (decode, compressed, checked) power {a.power}", t_decode)
    emit(f"verify_transform power {a.power}", total, **{k: round(v, 3) for k, v in sp.ms.items()})
