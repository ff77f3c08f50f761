#!/usr/bin/env python3
"""ECDSA / GOST R 34.10 verification benchmark (include/lcb_ecdsa_gpu.h),
device resident: HIP-event time per launch, warm-up excluded, median of
--reps launches, the engine clock of the timed launches themselves
(bench.ClockWindow).

Rows: valid signatures (made by tests/ecdsa_model.py from --keys distinct
keys, one signature each, repeated to the batch size, addressed through
key_idx) at 2^16 and 2^20 items on secp256r1, secp256k1 and CryptoPro-A; and
on secp256r1 a mix in which every second item has an off-curve key (-1: its
lane idles while its wave runs the ladder).  Every row's statuses are checked
once before it is timed.

CPU comparison: where oracle/_ref/libref_ecdsa.so exists (built by
tests/golden/make_golden_ecdsa.py; it travels with the tree) the reference's
own ecdsa_verify_be is timed on this box over the same records with 1 and 16
threads.  Where it does not, the rate the generator recorded in
tests/golden/ecdsa.json is printed, labelled as measured on another machine.

usage: python3 tools/ecdsa_bench.py [--reps 11] [--warmup 3] [--out profiles/ecdsa_bench.json]
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
from tests import ecdsa_model as M  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=11)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--keys", type=int, default=256)
p.add_argument("--counts", default="65536,1048576")
p.add_argument("--curves", default="secp256r1,secp256k1,id-gostR3410-2001-CryptoPro-A-ParamSet")
p.add_argument("--cpu-items", type=int, default=512, help="reference calls per thread in the CPU comparison")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 10, "the median of at least 10 repetitions"

FX = M.load_fixture()
CURVES = M.load_curves(FX)
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ecdsa.so")
s = torch.cuda.current_stream()
dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731


def records(name, le, nkeys):
    """nkeys (hash, sig, key) records, one valid signature per distinct key."""
    c = CURVES[name]
    rng = random.Random(0xBE7C)
    hashes, sigs, keys = [], [], []
    for _ in range(nkeys):
        d = rng.randrange(1, c["n"])
        Q = M.public_key(c, d)
        h = bytes(rng.randrange(256) for _ in range(32))
        r, sg = M.sign(c, h, 32, d, rng.randrange(1, 1 << 256), le)
        hashes.append(h)
        sigs.append(M.to_bytes(r, le) + M.to_bytes(sg, le))
        keys.append(M.to_bytes(Q[0], le) + M.to_bytes(Q[1], le))
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


def cpu_rates(name, le, hashes, sigs, keys):
    """The reference's ecdsa_verify_be (le: ecdsa_verify_le) per second on this box, 1 and 16 threads."""
    L = ctypes.CDLL(REF_SO)
    L.ref_ecdsa_load.argtypes = [ctypes.c_char_p]
    L.ref_ecdsa_verify_many.restype = ctypes.c_long
    slot = L.ref_ecdsa_load(name.encode())
    assert slot >= 0, name
    n = a.cpu_items
    idx = np.arange(n) % hashes.shape[0]
    recs = np.concatenate([hashes[idx], sigs[idx], keys[idx]], axis=1).reshape(-1)   # 160 bytes per record
    out = {}
    for threads in (1, 16):
        bufs = [(ctypes.c_uint8 * recs.size).from_buffer_copy(recs.tobytes()) for _ in range(threads)]
        bad = [None] * threads

        def work(t):
            bad[t] = L.ref_ecdsa_verify_many(slot, int(le), bufs[t], ctypes.c_size_t(n))

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


rows, cpu = {}, {}
for name in a.curves.split(","):
    le = CURVES[name]["algo"] == M.ALGO_GOST      # the natural form of the curve
    hashes, sigs, keys = records(name, le, a.keys)
    dkeys = dev(keys.reshape(-1))
    for count in [int(x) for x in a.counts.split(",")]:
        idx = np.arange(count, dtype=np.int32) % a.keys
        dh, dsg, di = dev(hashes[idx].reshape(-1)), dev(sigs[idx].reshape(-1)), dev(idx)
        out = torch.empty(count, dtype=torch.int32, device="cuda")
        mixes = [("valid", dkeys, np.zeros(count, np.int32))]
        if name == "secp256r1":
            bad = keys.copy()
            bad[:, 63 if not le else 32] ^= 1                  # Qy off the curve
            both = np.concatenate([keys, bad]).reshape(-1)     # key k valid, key nkeys + k not
            want = np.zeros(count, np.int32)
            want[1::2] = -1
            mixes.append(("half_offcurve", dev(both), want))
        for mix, dk, want in mixes:
            dmi = di if mix == "valid" else dev((idx + (np.arange(count) & 1) * a.keys).astype(np.int32))
            launch = lambda: E.verify_batch(name, dh, dsg, dk, key_idx=dmi, le=le, out=out)  # noqa: E731
            launch()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), (name, count, mix)
            ts, clock = timed(launch)
            med = ts[len(ts) // 2]
            row = "%s_%s_%d" % (name, mix, count)
            rows[row] = {"median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
                         "reps": a.reps, "verifies_per_s": round(count / (med * 1e-3)), "clock": clock}
            print("%-62s median %9.4f ms  min %9.4f  %12d verifies/s  clock %s GHz" % (
                row, med, ts[0], rows[row]["verifies_per_s"], clock and clock.get("clock_GHz")), flush=True)
    if os.path.exists(REF_SO):
        cpu[name] = cpu_rates(name, le, hashes, sigs, keys)
        print("%-62s reference ecdsa_verify_{be,le} on this box: %s verifies/s" % (name, cpu[name]), flush=True)
res = {"tag": a.tag, "keys": a.keys, "warmup": a.warmup, "rows": rows}
if cpu:
    res["reference_cpu_this_box"] = cpu
else:
    res["reference_cpu_other_machine"] = FX["ref_rate"]
    print("reference ecdsa_verify_be, measured on ANOTHER machine (the fixture's generator): %s" % FX["ref_rate"])
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
