#!/usr/bin/env python3
"""ECDSA / GOST R 34.10-2012 signing benchmark on the 384- and 512-bit curves
(include/lcb_ecdsa_wide_sign_gpu.h), the method of tools/ecdsa_wide_bench.py:
device resident, HIP-event time per launch, warm-up excluded, median of --reps
launches, the engine clock of the timed launches themselves
(bench.ClockWindow).

Rows, per curve (secp384r1 and brainpoolP512r1 in the be form, paramSetA in
the le form) and batch size (2^16, 2^20): key_gen_batch over random bytes,
then sign_batch of random hashes with the generated keys and fresh nonces,
then pub_key_batch of the generated keys, and in the same session
ecdsa_wide.verify_batch (liblcb_ecdsa_wide_gpu.so, unchanged) over the
signatures just made.  The control rows are the 256-bit secp256r1 sign
(liblcb_ecdsa_sign_gpu.so, unchanged), made and timed the same way.  Before
any timing every status must be 0, the verification of the signatures must be
0 and pub_key_batch must return the generated public keys.  At the largest
batch size signing must be faster than the verification of the same curve:
the run fails where it is not.

CPU comparison: where oracle/_ref/libref_ecdsa_wide_sign.so exists (built by
tests/golden/make_golden_ecdsa_wide_sign.py; it travels with the tree) the
reference's own ecdsa_sign_be / _le is timed on this box over the first
records with 1 and 16 threads.  Where it does not, the rate the generator
recorded in tests/golden/ecdsa_wide_sign.json is printed, labelled as measured
on another machine.

usage: python3 tools/ecdsa_wide_sign_bench.py [--reps 11] [--warmup 3] [--out profiles/ecdsa_wide_sign_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ClockWindow  # noqa: E402
from liblcb_amd import ecdsa_sign as S8  # noqa: E402
from liblcb_amd import ecdsa_wide as W  # noqa: E402
from liblcb_amd import ecdsa_wide_sign as S  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=11)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--counts", default="65536,1048576")
p.add_argument("--curves", default="secp384r1,brainpoolP512r1,id-tc26-gost-3410-12-512-paramSetA")
p.add_argument("--control", default="secp256r1")
p.add_argument("--cpu-items", type=int, default=512, help="reference calls per thread in the CPU comparison")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 10, "the median of at least 10 repetitions"

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ecdsa_wide_sign.so")
COUNTS = [int(x) for x in a.counts.split(",")]
s = torch.cuda.current_stream()
dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731


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


def cpu_rates(name, le, B, hashes, priv, rnd):
    """The reference's ecdsa_sign_be (le: ecdsa_sign_le) per second on this box, 1 and 16 threads."""
    L = ctypes.CDLL(REF_SO)
    L.ref_wide_sign_load.argtypes = [ctypes.c_char_p]
    L.ref_wide_sign_bytes.restype = ctypes.c_size_t
    L.ref_wide_sign_many.restype = ctypes.c_long
    slot = L.ref_wide_sign_load(name.encode())
    assert slot >= 0 and L.ref_wide_sign_bytes(slot) == B, name
    n = a.cpu_items
    recs = np.concatenate([hashes[:n], priv[:n], rnd[:n]], axis=1).reshape(-1)   # 3 B bytes per record
    out = {}
    for threads in (1, 16):
        bufs = [(ctypes.c_uint8 * recs.size).from_buffer_copy(recs.tobytes()) for _ in range(threads)]
        bad = [None] * threads

        def work(t):
            bad[t] = L.ref_wide_sign_many(slot, int(le), bufs[t], ctypes.c_size_t(n))

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


def record(row, count, ts, clock):
    med = ts[len(ts) // 2]
    rows[row] = {"count": count, "median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
                 "reps": a.reps, "items_per_s": round(count / (med * 1e-3)), "clock": clock}
    print("%-62s median %10.4f ms  min %10.4f  %12d items/s  clock %s GHz" % (
        row, med, ts[0], rows[row]["items_per_s"], clock and clock.get("clock_GHz")), flush=True)


rows, cpu = {}, {}
rng = np.random.default_rng(0x516E512)
# the control: the 256-bit signing library, unchanged
for count in COUNTS:
    seed, nonce, hashes = (dev(rng.integers(0, 256, 32 * count, dtype=np.uint8)) for _ in range(3))
    priv, pub, kst = S8.key_gen_batch(a.control, seed)
    osig = torch.empty(64 * count, dtype=torch.uint8, device="cuda")
    ost = torch.empty(count, dtype=torch.int32, device="cuda")
    launch = lambda: S8.sign_batch(a.control, hashes, priv.reshape(-1), nonce, out=(osig, ost))  # noqa: E731
    launch()
    torch.cuda.synchronize()
    assert not kst.any().item() and not ost.any().item(), (a.control, count)
    record("%s_sign_%d" % (a.control, count), count, *timed(launch))

for name in a.curves.split(","):
    B = W.curve_bytes(name)
    le = W.curve_params(name)["algo"] == W.ALGO_GOST      # the natural form of the curve
    for count in COUNTS:
        seed, nonce, hashes = (rng.integers(0, 256, (count, B), dtype=np.uint8) for _ in range(3))
        dseed, dnonce, dh = dev(seed.reshape(-1)), dev(nonce.reshape(-1)), dev(hashes.reshape(-1))
        priv, pub, kst = S.key_gen_batch(name, dseed, le=le)
        dpriv, dpub = priv.reshape(-1), pub.reshape(-1)
        osig = torch.empty(2 * B * count, dtype=torch.uint8, device="cuda")
        ost = torch.empty(count, dtype=torch.int32, device="cuda")
        vst = torch.empty(count, dtype=torch.int32, device="cuda")
        sigs, sst = S.sign_batch(name, dh, dpriv, dnonce, le=le, out=(osig, ost))
        pub2, pst = S.pub_key_batch(name, dpriv, le=le)
        W.verify_batch(name, dh, osig, dpub, le=le, out=vst)
        torch.cuda.synchronize()
        for what, st in (("key_gen", kst), ("sign", sst), ("pub_key", pst), ("verify", vst)):
            assert not st.any().item(), (name, count, what, st[st != 0][:8].tolist())
        assert torch.equal(pub2, pub), (name, count)
        ops = (("sign", lambda: S.sign_batch(name, dh, dpriv, dnonce, le=le, out=(osig, ost))),
               ("key_gen", lambda: S.key_gen_batch(name, dseed, le=le)),
               ("pub_key", lambda: S.pub_key_batch(name, dpriv, le=le)),
               ("verify", lambda: W.verify_batch(name, dh, osig, dpub, le=le, out=vst)))
        for op, launch in ops:
            record("%s_%s_%d" % (name, op, count), count, *timed(launch))
        assert not ost.any().item() and not vst.any().item()      # the timed launches wrote the same answers
        r = rows["%s_sign_%d" % (name, count)]
        r["control_over_this"] = round(rows["%s_sign_%d" % (a.control, count)]["items_per_s"] / r["items_per_s"], 2)
        r["over_verify"] = round(r["items_per_s"] / rows["%s_verify_%d" % (name, count)]["items_per_s"], 2)
        print("%-62s control / this %6.2f   this / verify %6.2f" % ("%s_sign_%d" % (name, count),
                                                                     r["control_over_this"], r["over_verify"]))
    if os.path.exists(REF_SO):
        cpu[name] = cpu_rates(name, le, B, hashes, priv.cpu().numpy(), nonce)
        print("%-62s reference ecdsa_sign_{be,le} on this box: %s signs/s" % (name, cpu[name]), flush=True)
res = {"tag": a.tag, "warmup": a.warmup, "control": a.control, "rows": rows}
if cpu:
    res["reference_cpu_this_box"] = cpu
else:
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ecdsa_wide_sign.json")))
    res["reference_cpu_other_machine"] = fx["ref_rate"]
    print("reference ecdsa_sign, measured on ANOTHER machine (the fixture's generator): %s" % fx["ref_rate"])
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
# The acceptance condition: a signature is a quarter of a verification's products.
slow = [name for name in a.curves.split(",")
        if rows["%s_sign_%d" % (name, COUNTS[-1])]["over_verify"] <= 1.0]
assert not slow, "signing is not faster than verification at %d items: %s" % (COUNTS[-1], slow)
