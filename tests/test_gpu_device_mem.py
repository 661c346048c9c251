"""The library's device memory (csrc/device_mem.hpp: grow-only buffers, the per-stream scratch, the leased pools) through its release and growth paths.

Release, then use again: one call through every owner of device memory -- a two-pass fft (the inter-pass scratch; the size is the smallest one ntt_plan
cuts into two passes, read from tests/cpp/test_ntt_host.cpp's dump) and a single-pass one, G1 / G2 batch_exp over 64 points and batch_mul over 64 scalars
(the scalar-multiplication scratch, the slot rings), a device G1 multiexp at 2^10 (small workspaces, pinned buffers), a host-buffer one over pinned bases
(bases cache, stage pool), a host-array fft at 2^10 (the device buffer pool), a 16-point decode and a 2^4 point fft (per-call temporaries) -- each against
the oracle; then mi355zk_shutdown, mi355zk_init and all of them twice more: the first round meets empty pools, the second refilled ones.

Growth: on one stream batch_exp at 64, 4096 and 64 points and a two-pass fft, the next size up and the first size again: the regrow behind a stream
synchronisation and a smaller call in a larger buffer.

Each runs in a fresh child process (it shuts the library down) under a timeout of its own."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120


def _two_pass_log_n():
    """the smallest log_n whose plain transform the planner cuts into two passes, from ntt_plan.hpp under this process's knobs"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "test_ntt_host_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_ntt_host.cpp"), "-o", exe])
    passes = {}
    for line in subprocess.run([exe, "dump"], capture_output=True, text=True, check=True).stdout.splitlines():
        head, _, plan = line.partition(": ")
        if " batch=1 pre_g=0 post_c=0 post_g=0" in head and " rc=0 " in " " + plan:
            passes[int(head.split()[0].split("=")[1])] = int(plan.split(" R=")[1].split()[0])
    two = min(l for l, r in passes.items() if r == 2)
    assert passes[two - 1] == 1 and passes[two + 1] == 2
    return two


def _run_child(mode):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), mode, str(_two_pass_log_n())]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok " + mode), "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


def test_every_pool_is_usable_after_shutdown():
    out = _run_child("release")
    assert out.count("round ") == 3 and out.count("shutdown") == 1


def test_scratch_grows_behind_its_stream_and_serves_smaller_calls():
    _run_child("growth")


# ------------------------------------------------------------------------------------------------ the child process
def _steps(two_pass, worker):
    """{name: run}: every run() makes one call and compares it with an expectation computed here, once, on the CPU"""
    import ctypes as C

    import numpy as np
    import torch

    import bn254_model as M
    import inputs
    import oracle_lib as O
    import phase2_bn254_amd as zk

    L = zk.lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()  # noqa: E731
    host = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    steps = {}

    def fft(log_n, seed):
        a = inputs.random_fr_mont(1 << log_n, seed=seed)
        want = O.fr_domain_op(a, log_n, "fft").reshape(-1, 4)

        def run():
            dom = zk.EvaluationDomain.from_coeffs(dev(a))
            dom.fft(worker)
            assert np.array_equal(host(dom.into_coeffs()), want), ("fft", log_n)
        return run

    for name, log_n in (("fft two-pass", two_pass), ("fft two-pass, next size", two_pass + 1), ("fft single-pass", two_pass - 1)):
        steps[name] = fft(log_n, 9100 + log_n)

    # k * (P + i S) = k P + i (k S): the oracle multiplies two points, whatever n is
    k = np.array([M.to_limbs(0x1234567890ABCDEF1234567890ABCDEF0FEDCBA987654321)], dtype=np.uint64)
    d_k = dev(k)
    for g, G, gen, n_max in ((1, O.G1, inputs.G1_GEN_RAW, 4096), (2, O.G2, inputs.G2_GEN_RAW, 64)):
        bases = inputs.bases_progression_cpu(g, n_max, seed=9200 + g)
        step = G.mul_many_affine(gen, inputs.random_scalars(2, 9200 + g))[1]
        assert np.array_equal(G.arith_progression_affine(bases[0], step, 3), bases[:3])
        kp, ks = (G.to_affine(G.mul(G.from_affine(p), k[0])) for p in (bases[0], step))
        want = G.arith_progression_affine(kp, ks, n_max)
        d_b = dev(bases)

        def exp(n, d_b=d_b, want=want, g=g):
            def run():
                out = zk.ceremony.batch_exp(d_b[:n].contiguous(), d_k, same_scalar=True)
                assert np.array_equal(host(out), want[:n]), ("batch_exp", g, n)
            return run

        steps["batch_exp g%d 64" % g] = exp(64)
        if g == 1:
            steps["batch_exp g1 4096"] = exp(4096)

        sc = inputs.random_scalars(64, seed=9210 + g)
        want_mul = G.mul_many_affine(gen, sc)
        d_sc, gen_c = dev(sc), np.ascontiguousarray(gen)

        def mul(g=g, d_sc=d_sc, gen_c=gen_c, want_mul=want_mul):
            out = torch.empty((64, 8 * g), dtype=torch.int64, device="cuda")
            fn = L.mi355zk_bn254_g1_batch_mul_dev if g == 1 else L.mi355zk_bn254_g2_batch_mul_dev
            assert fn(C.c_void_p(out.data_ptr()), gen_c.ctypes.data_as(C.c_void_p), C.c_void_p(d_sc.data_ptr()), 64, None) == 0
            assert np.array_equal(host(out), want_mul), ("batch_mul", g)
        steps["batch_mul g%d" % g] = mul

    n = 1 << 10
    bases_d, bases_h = inputs.bases_progression_cpu(1, n, seed=9300), inputs.bases_progression_cpu(1, n, seed=9301)
    scalars = inputs.random_scalars(n, seed=9302)
    wants = []
    for b in (bases_d, bases_h):
        rc, w = O.G1.multiexp(b, scalars, threads=4)
        assert rc == 0
        wants.append(O.G1.to_affine(w))
    d_bases, d_scalars = dev(bases_d), dev(scalars)
    zk.pin_bases(bases_h)   # (bases_h stays alive in run's closure)

    def msm_dev():
        got = zk.multiexp(worker, (d_bases, 0), zk.FullDensity(), d_scalars).wait()
        assert np.array_equal(O.G1.to_affine(got), wants[0]), "device multiexp"

    def msm_host():
        got = zk.multiexp(worker, (bases_h, 0), zk.FullDensity(), scalars).wait()
        assert np.array_equal(O.G1.to_affine(got), wants[1]), "host-buffer multiexp"
    steps["multiexp g1 2^10, device"], steps["multiexp g1 2^10, host buffers"] = msm_dev, msm_host

    a10 = inputs.random_fr_mont(n, seed=9400)
    want10 = O.fr_domain_op(a10, 10, "fft").reshape(-1, 4)

    def fft_host():
        dom = zk.EvaluationDomain.from_coeffs(a10)
        dom.fft(worker)
        assert np.array_equal(dom.into_coeffs(), want10), "host-array fft"
    steps["fft 2^10, host array"] = fft_host

    pts = inputs.bases_progression_cpu(1, 16, seed=9500)
    enc = torch.from_numpy(np.ascontiguousarray(O.encode_points(1, pts, True))).cuda()
    want_pfft = O.point_domain_op(1, pts, 4, "fft")

    def decode():
        assert np.array_equal(host(zk.ceremony.decode_points(enc, 1, compressed=True)), pts), "decode"

    def point_fft():
        d = dev(pts)
        assert L.mi355zk_bn254_g1_point_fft_dev(C.c_void_p(d.data_ptr()), 4, 0, None) == 0
        assert np.array_equal(host(d), want_pfft), "point fft"
    steps["decode g1 16"], steps["point fft g1 2^4"] = decode, point_fft
    return steps


RELEASE_ROUND = ["fft two-pass", "fft single-pass", "batch_exp g1 64", "batch_exp g2 64", "batch_mul g1", "batch_mul g2", "multiexp g1 2^10, device",
                 "multiexp g1 2^10, host buffers", "fft 2^10, host array", "decode g1 16", "point fft g1 2^4"]
GROWTH = ["batch_exp g1 64", "batch_exp g1 4096", "batch_exp g1 64", "fft two-pass", "fft two-pass, next size", "fft two-pass"]


def _child(mode, two_pass):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import phase2_bn254_amd as zk

    worker = zk.Worker(0)
    steps = _steps(two_pass, worker)
    torch.cuda.synchronize()
    if mode == "growth":
        with torch.cuda.stream(torch.cuda.Stream()):   # one stream for all six: the scratch is per (device, stream)
            for name in GROWTH:
                steps[name]()
                print("passed", name, flush=True)
    else:
        for rnd in range(3):
            print("round %d" % rnd, flush=True)
            for name in RELEASE_ROUND:
                steps[name]()
                print("passed", name, flush=True)
            if rnd == 0:
                torch.cuda.synchronize()
                zk.lib.load().mi355zk_shutdown()
                print("shutdown", flush=True)
                worker = zk.Worker(0)   # mi355zk_init
    torch.cuda.synchronize()
    print("ok " + mode, flush=True)


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
