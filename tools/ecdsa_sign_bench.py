#!/usr/bin/env python3
"""ECDSA / GOST R 34.10 signing benchmark (include/lcb_ecdsa_sign_gpu.h),
device resident: HIP-event time per launch, warm-up excluded, median of
--reps launches, the engine clock of the timed launches themselves
(bench.ClockWindow).

Rows, per curve (secp256r1, secp256k1 in the be form, CryptoPro-A in the le
form) and batch size (2^16, 2^20): key_gen_batch over random bytes, then
sign_batch of random hashes with the generated keys and fresh nonces, then
pub_key_batch of the generated keys, and as the baseline verify_batch
(liblcb_ecdsa_gpu.so, unchanged) over the signatures just made.  Before any
timing every status must be 0, the verification of the signatures must be 0
and pub_key_batch must return the generated public keys.

CPU comparison: where oracle/_ref/libref_ecdsa_sign.so exists (built by
tests/golden/make_golden_ecdsa_sign.py; it travels with the tree) the
reference's own ecdsa_sign_be / _le is timed on this box over the first
records with 1 and 16 threads.  Where it does not, the rate the generator
recorded in tests/golden/ecdsa_sign.json is printed, labelled as measured on
another machine.

usage: python3 tools/ecdsa_sign_bench.py [--reps 11] [--warmup 3] [--out profiles/ecdsa_sign_bench.json]
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
from liblcb_amd import ecdsa as E  # noqa: E402
from liblcb_amd import ecdsa_sign as S  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=11)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--counts", default="65536,1048576")
p.add_argument("--curves", default="secp256r1,secp256k1,id-gostR3410-2001-CryptoPro-A-ParamSet")
p.add_argument("--cpu-items", type=int, default=2048, help="reference calls per thread in the CPU comparison")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 10, "the median of at least 10 repetitions"

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ecdsa_sign.so")
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


def cpu_rates(name, le, hashes, priv, rnd):
    """The reference's ecdsa_sign_be (le: ecdsa_sign_le) per second on this box, 1 and 16 threads."""
    L = ctypes.CDLL(REF_SO)
    L.ref_sign_load.argtypes = [ctypes.c_char_p]
    L.ref_sign_many.restype = ctypes.c_long
    slot = L.ref_sign_load(name.encode())
    assert slot >= 0, name
    n = a.cpu_items
    recs = np.concatenate([hashes[:n], priv[:n], rnd[:n]], axis=1).reshape(-1)   # 96 bytes per record
    out = {}
    for threads in (1, 16):
        bufs = [(ctypes.c_uint8 * recs.size).from_buffer_copy(recs.tobytes()) for _ in range(threads)]
        bad = [None] * threads

        def work(t):
            bad[t] = L.ref_sign_many(slot, int(le), bufs[t], ctypes.c_size_t(n))

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
rng = np.random.default_rng(0x516E)
for name in a.curves.split(","):
    le = E.curve_params(name)["algo"] == E.ALGO_GOST      # the natural form of the curve
    for count in [int(x) for x in a.counts.split(",")]:
        seed, nonce, hashes = (rng.integers(0, 256, (count, 32), dtype=np.uint8) for _ in range(3))
        dseed, dnonce, dh = dev(seed.reshape(-1)), dev(nonce.reshape(-1)), dev(hashes.reshape(-1))
        priv, pub, kst = S.key_gen_batch(name, dseed, le=le)
        dpriv, dpub = priv.reshape(-1), pub.reshape(-1)
        osig = torch.empty(64 * count, dtype=torch.uint8, device="cuda")
        ost = torch.empty(count, dtype=torch.int32, device="cuda")
        vst = torch.empty(count, dtype=torch.int32, device="cuda")
        sigs, sst = S.sign_batch(name, dh, dpriv, dnonce, le=le, out=(osig, ost))
        pub2, pst = S.pub_key_batch(name, dpriv, le=le)
        E.verify_batch(name, dh, osig, dpub, le=le, out=vst)
        torch.cuda.synchronize()
        for what, st in (("key_gen", kst), ("sign", sst), ("pub_key", pst), ("verify", vst)):
            assert not st.any().item(), (name, count, what, st[st != 0][:8].tolist())
        assert torch.equal(pub2, pub), (name, count)
        ops = (("sign", lambda: S.sign_batch(name, dh, dpriv, dnonce, le=le, out=(osig, ost))),
               ("key_gen", lambda: S.key_gen_batch(name, dseed, le=le)),
               ("pub_key", lambda: S.pub_key_batch(name, dpriv, le=le)),
               ("verify", lambda: E.verify_batch(name, dh, osig, dpub, le=le, out=vst)))
        for op, launch in ops:
            ts, clock = timed(launch)
            med = ts[len(ts) // 2]
            row = "%s_%s_%d" % (name, op, count)
            rows[row] = {"median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
                         "reps": a.reps, "items_per_s": round(count / (med * 1e-3)), "clock": clock}
            print("%-62s median %9.4f ms  min %9.4f  %12d items/s  clock %s GHz" % (
                row, med, ts[0], rows[row]["items_per_s"], clock and clock.get("clock_GHz")), flush=True)
        assert not ost.any().item() and not vst.any().item()      # the timed launches wrote the same answers
    if os.path.exists(REF_SO):
        cpu[name] = cpu_rates(name, le, hashes, priv.cpu().numpy(), nonce)
        print("%-62s reference ecdsa_sign_{be,le} on this box: %s signs/s" % (name, cpu[name]), flush=True)
res = {"tag": a.tag, "warmup": a.warmup, "rows": rows}
if cpu:
    res["reference_cpu_this_box"] = cpu
else:
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ecdsa_sign.json")))
    res["reference_cpu_other_machine"] = fx["ref_rate"]
    print("reference ecdsa_sign_be, measured on ANOTHER machine (the fixture's generator): %s" % fx["ref_rate"])
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
