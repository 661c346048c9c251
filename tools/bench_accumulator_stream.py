#!/usr/bin/env python3
"""Powers-of-tau files streamed through one MI355X against the in-memory flows on the same bytes -> profiles/accumulator_stream.md.

At --power (20: a 384 MiB challenge) the tool makes a challenge with non-trivial points (new_constrained -> compute_constrained ->
verify_transform_constrained: the new challenge of a first contribution), then times on that challenge

  streamed   compute_constrained and verify_transform_constrained, file to file, split into hashing (calculate_hash_file, every call of it:
             some run on a helper thread beside the device), device pipeline (the chunks' accumulator_transform / accumulator_power_pairs calls)
             and total;
  in memory  contribute_response and read_response + verify_transform + next_challenge on the same bytes already read into host memory
             (reading and writing the files is not charged to them).

Times are medians of --iters runs after --warm runs, in ms; no figure is a gate."""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--power", type=int, default=20); ap.add_argument("--batch-size", type=int, default=1 << 18); ap.add_argument("--piece", type=int, default=0)
ap.add_argument("--iters", type=int, default=3); ap.add_argument("--warm", type=int, default=1); ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulator_stream.md"))
a = ap.parse_args()

import numpy as np, torch  # noqa: E402
import phase2_bn254_amd as zk  # noqa: E402
zk.lib.load(); zk.Worker(0)
KEY = bytes(range(32))
SECRETS = (0xABCDEF123456789, 0x1111222233334444, 0x9999AAAABBBB)
spent = {"hashing": 0.0, "device pipeline": 0.0}


def charged(name, fn):
    def wrapper(*args, **kwargs):
        t = time.perf_counter()
        try:
            return fn(*args, **kwargs)
        finally:
            spent[name] += (time.perf_counter() - t) * 1e3
    return wrapper


zk.stream.calculate_hash_file = charged("hashing", zk.stream.calculate_hash_file)
zk.stream._run = charged("device pipeline", zk.stream._run)


def timed(fn):
    """medians of the total and of the two charged parts"""
    rows = []
    for i in range(a.warm + a.iters):
        for k in spent: spent[k] = 0.0
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize()
        rows.append({"total": (time.perf_counter() - t) * 1e3, **spent})
    rows = rows[a.warm:]
    return {k: round(statistics.median(r[k] for r in rows), 1) for k in rows[0]}


with tempfile.TemporaryDirectory(dir=a.dir) as d:
    p = lambda name: os.path.join(d, name)  # noqa: E731
    zk.new_constrained(p("challenge0"), a.power, a.batch_size)
    zk.compute_constrained(p("challenge0"), p("response1"), a.power, a.batch_size, *SECRETS, piece=a.piece)
    zk.verify_transform_constrained(p("challenge0"), p("response1"), p("challenge1"), a.power, a.batch_size, key=KEY, piece=a.piece)
    sizes = {name: os.path.getsize(p(name)) for name in ("challenge1", "response1")}
    results = []
    results.append(("compute_constrained (streamed, file to file)",
                    timed(lambda: zk.compute_constrained(p("challenge1"), p("response2"), a.power, a.batch_size, *SECRETS, piece=a.piece))))
    results.append(("verify_transform_constrained (streamed, file to file)",
                    timed(lambda: zk.verify_transform_constrained(p("challenge1"), p("response2"), p("challenge2"), a.power, a.batch_size, key=KEY, piece=a.piece))))
    challenge = open(p("challenge1"), "rb").read()
    response = open(p("response2"), "rb").read()
    results.append(("contribute_response (in memory)", timed(lambda: zk.contribute_response(challenge, a.power, *SECRETS))))

    def verify_in_memory():
        before = zk.ceremony.read_accumulator(zk.verify._file_tensor(challenge), a.power, compressed=False)
        after, pub = zk.verify.read_response(response, a.power)
        zk.verify_transform(before, after, pub, zk.ceremony.calculate_hash(np.frombuffer(challenge, dtype=np.uint8)), key=KEY)
        zk.next_challenge(response, a.power)

    results.append(("read_accumulator + read_response + verify_transform + next_challenge (in memory)", timed(verify_in_memory)))
    peak = torch.cuda.max_memory_allocated()

with open(a.out, "w") as f:
    f.write("# Streamed accumulator files: measurements\n\nWritten by `tools/bench_accumulator_stream.py --power %d --batch-size %d --piece %d` on %s: medians of %d runs "
            "after %d warm-up runs, ms.  Challenge %.0f MiB, response %.0f MiB.  `hashing` adds up every calculate_hash_file of the call (the challenge's "
            "runs beside the device in compute_constrained, the response's beside it in verify_transform_constrained, the written file's after it); "
            "`device pipeline` is the wall time of the chunks' accumulator calls.\n\n| flow | total | hashing | device pipeline |\n|---|---|---|---|\n"
            % (a.power, a.batch_size, a.piece, torch.cuda.get_device_name(0), a.iters, a.warm, sizes["challenge1"] / 2**20, sizes["response1"] / 2**20))
    for what, r in results:
        streamed = "streamed" in what
        f.write("| %s | %s | %s | %s |\n" % (what, r["total"], r["hashing"] if streamed else "(inside)", r["device pipeline"] if streamed else "(inside)"))
    f.write("\nPeak of torch's allocator over the in-memory flows: %.0f MiB (the streamed calls allocate through the library's pools, a fixed multiple of the piece).\n" % (peak / 2**20))
for what, r in results:
    print(json.dumps({"what": what, **r}), flush=True)
