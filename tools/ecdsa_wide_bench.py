#!/usr/bin/env python3
"""ECDSA / GOST R 34.10-2012 verification benchmark on the 384- and 512-bit
curves (include/lcb_ecdsa_wide_gpu.h), the method of tools/ecdsa_bench.py:
device resident, HIP-event time per launch, warm-up excluded, median of --reps
launches, the engine clock of the timed launches themselves
(bench.ClockWindow).

Rows: valid signatures (made by tests/ecdsa_wide_model.py from --keys distinct
keys, one signature each, repeated to the batch size, addressed through
key_idx) at 2^16 and 2^20 items on secp384r1, brainpoolP512r1 and
id-tc26-gost-3410-12-512-paramSetA, each in its natural form; and the control
row, secp256r1 through the 256-bit library (liblcb_amd.ecdsa), made and timed
the same way in the same session.  Every row's statuses are checked once
before it is timed; the ratio of every row to the control row of its batch
size is printed.

CPU comparison: where oracle/_ref/libref_ecdsa_wide.so exists (built by
tests/golden/make_golden_ecdsa_wide.py; it travels with the tree) the
reference's own ecdsa_verify_{be,le} is timed on this box over the same
records with 1 and 16 threads.  Where it does not, the rate the generator
recorded in tests/golden/ecdsa_wide.json is printed, labelled as measured on
another machine.

usage: python3 tools/ecdsa_wide_bench.py [--reps 11] [--warmup 3] [--out profiles/ecdsa_wide_bench.json]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ClockWindow  # noqa: E402
from liblcb_amd import ecdsa as E  # noqa: E402
from liblcb_amd import ecdsa_wide as W  # noqa: E402
from tests import ecdsa_model as M8  # noqa: E402
from tests import ecdsa_wide_model as M  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=11)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--keys", type=int, default=64)
p.add_argument("--counts", default="65536,1048576")
p.add_argument("--curves", default="secp384r1,brainpoolP512r1,id-tc26-gost-3410-12-512-paramSetA")
p.add_argument("--control", default="secp256r1")
p.add_argument("--cpu-items", type=int, default=128, help="reference calls per thread in the CPU comparison")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 10, "the median of at least 10 repetitions"

FX = M.load_fixture()
CURVES = M.load_curves(FX)
CURVES8 = M8.load_curves()
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ecdsa_wide.so")
s = torch.cuda.current_stream()
dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731


def records(c, B, le, nkeys, sign, public_key, to_bytes):
    """nkeys (hash, sig, key) records, one valid signature per distinct key."""
    rng = random.Random(0xBE7C)
    hashes, sigs, keys = [], [], []
    for _ in range(nkeys):
        d = rng.randrange(1, c["n"])
        Q = public_key(c, d)
        h = bytes(rng.randrange(256) for _ in range(B))
        r, sg = sign(c, h, B, d, rng.randrange(1, 1 << (8 * B)), le)
        hashes.append(h)
        sigs.append(to_bytes(r) + to_bytes(sg))
        keys.append(to_bytes(Q[0]) + to_bytes(Q[1]))
    f = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(nkeys, -1).copy()  # noqa: E731
    return f(hashes), f(sigs), f(keys)


def timed(launch):
    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    cw = ClockWindow(s)
    cw.begin()
    evs = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        launch()
        e1.record(s)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    cw.end()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts, cw.result(busy_ms=sum(ts))


def cpu_rates(name, le, B, hashes, sigs, keys):
    """The reference's ecdsa_verify_{be,le} per second on this box, 1 and 16 threads."""
    L = ctypes.CDLL(REF_SO)
    L.ref_ecdsa_wide_load.argtypes = [ctypes.c_char_p]
    L.ref_ecdsa_wide_verify_many.restype = ctypes.c_long
    slot = L.ref_ecdsa_wide_load(name.encode())
    assert slot >= 0, name
    n = a.cpu_items
    idx = np.arange(n) % hashes.shape[0]
    recs = np.concatenate([hashes[idx], sigs[idx], keys[idx]], axis=1).reshape(-1)   # 5 B bytes per record
    out = {}
    for threads in (1, 16):
        bufs = [(ctypes.c_uint8 * recs.size).from_buffer_copy(recs.tobytes()) for _ in range(threads)]
        bad = [None] * threads

        def work(t):
            bad[t] = L.ref_ecdsa_wide_verify_many(slot, int(le), bufs[t], ctypes.c_size_t(n))

        ths = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        assert bad == [0] * threads, bad
        out["threads_%d" % threads] = round(threads * n / dt, 1)
    return out


def bench_curve(name, mod, c, B, le, sign, public_key, to_bytes):
    hashes, sigs, keys = records(c, B, le, a.keys, sign, public_key, to_bytes)
    dkeys = dev(keys.reshape(-1))
    for count in [int(x) for x in a.counts.split(",")]:
        idx = np.arange(count, dtype=np.int32) % a.keys
        dh, dsg, di = dev(hashes[idx].reshape(-1)), dev(sigs[idx].reshape(-1)), dev(idx)
        out = torch.empty(count, dtype=torch.int32, device="cuda")
        launch = lambda: mod.verify_batch(name, dh, dsg, dkeys, key_idx=di, le=le, out=out)  # noqa: E731
        launch()
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any(), (name, count)
        ts, clock = timed(launch)
        med = ts[len(ts) // 2]
        row = "%s_valid_%d" % (name, count)
        rows[row] = {"bits": 8 * B, "count": count, "median_ms": round(med, 4), "min_ms": round(ts[0], 4),
                     "max_ms": round(ts[-1], 4), "reps": a.reps, "verifies_per_s": round(count / (med * 1e-3)),
                     "clock": clock}
        print("%-58s median %10.4f ms  min %10.4f  %11d verifies/s  clock %s GHz" % (
            row, med, ts[0], rows[row]["verifies_per_s"], clock and clock.get("clock_GHz")), flush=True)
    return hashes, sigs, keys


rows, cpu = {}, {}
c8 = CURVES8[a.control]
bench_curve(a.control, E, c8, 32, False, M8.sign, M8.public_key, lambda v: M8.to_bytes(v, False))
for name in a.curves.split(","):
    c = CURVES[name]
    le = c["algo"] == M.ALGO_GOST      # the natural form of the curve
    hashes, sigs, keys = bench_curve(name, W, c, c["bytes"], le, M.sign, M.public_key,
                                     lambda v, c=c, le=le: M.to_bytes(c, v, le))
    if os.path.exists(REF_SO):
        cpu[name] = cpu_rates(name, le, c["bytes"], hashes, sigs, keys)
        print("%-58s reference ecdsa_verify_{be,le} on this box: %s verifies/s" % (name, cpu[name]), flush=True)
for row, r in rows.items():
    ctl = rows["%s_valid_%d" % (a.control, r["count"])]
    r["control_over_this"] = round(ctl["verifies_per_s"] / r["verifies_per_s"], 2)
    print("%-58s the control row is %6.2f x as fast" % (row, r["control_over_this"]))
res = {"tag": a.tag, "keys": a.keys, "warmup": a.warmup, "control": a.control, "rows": rows}
if cpu:
    res["reference_cpu_this_box"] = cpu
else:
    res["reference_cpu_other_machine"] = FX["ref_rate"]
    print("reference ecdsa_verify, measured on ANOTHER machine (the fixture's generator): %s" % FX["ref_rate"])
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
