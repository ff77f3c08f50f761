#!/usr/bin/env python3
"""ECDH key agreement benchmark (include/lcb_ecdsa_dh_gpu.h), device
resident: HIP-event time per launch, warm-up excluded, median of --reps
launches, the engine clock of the timed launches themselves
(bench.ClockWindow).

Rows, per curve (secp256r1, secp256k1 in the be form, CryptoPro-A in the le
form) and batch size (2^16, 2^20): dh_batch of one private key (npriv = 1, a
priv_idx of zeros) against `count` peers whose public keys pub_key_batch made
on the device, and as the nearest kernel by instruction count verify_batch
(liblcb_ecdsa_gpu.so, unchanged) over as many signatures, made by sign_batch
in the same run.  Before any timing every status must be 0 and the first
secrets must equal the Python-int model's.

CPU comparison: where oracle/_ref/libref_ecdsa_dh.so exists (built by
tests/golden/make_golden_ecdsa_dh.py; it travels with the tree) the
reference's own ecdsa_dh_be / _le is timed on this box over the first records
with 1 and 16 threads.  Where it does not, the rate the generator recorded in
tests/golden/ecdsa_dh.json is printed, labelled as measured on another
machine.

usage: python3 tools/ecdsa_dh_bench.py [--reps 11] [--warmup 3] [--out profiles/ecdsa_dh_bench.json]
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
from liblcb_amd import ecdsa_dh as D  # noqa: E402
from liblcb_amd import ecdsa_sign as S  # noqa: E402
from tests import ecdsa_model as M  # noqa: E402

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

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ecdsa_dh.so")
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


def cpu_rates(name, le, pub, priv):
    """The reference's ecdsa_dh_be (le: ecdsa_dh_le) per second on this box, 1 and 16 threads."""
    L = ctypes.CDLL(REF_SO)
    L.ref_dh_load.argtypes = [ctypes.c_char_p]
    L.ref_dh_many.restype = ctypes.c_long
    slot = L.ref_dh_load(name.encode())
    assert slot >= 0, name
    n = a.cpu_items
    recs = np.concatenate([pub[:n], np.broadcast_to(priv, (n, 32))], axis=1).reshape(-1)   # 96 bytes per record
    out = {}
    for threads in (1, 16):
        bufs = [(ctypes.c_uint8 * recs.size).from_buffer_copy(recs.tobytes()) for _ in range(threads)]
        bad = [None] * threads

        def work(t):
            bad[t] = L.ref_dh_many(slot, int(le), bufs[t], ctypes.c_size_t(n))

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
rng = np.random.default_rng(0xD16E)
curves = M.load_curves()
for name in a.curves.split(","):
    c = curves[name]
    le = E.curve_params(name)["algo"] == E.ALGO_GOST      # the natural form of the curve
    for count in [int(x) for x in a.counts.split(",")]:
        seed, nonce, hashes = (rng.integers(0, 256, (count, 32), dtype=np.uint8) for _ in range(3))
        dh = dev(hashes.reshape(-1))
        peer_priv, pub, kst = S.key_gen_batch(name, dev(seed.reshape(-1)), le=le)
        dpub = pub.reshape(-1)
        dval = M.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), False) % (c["n"] - 1) + 1
        mine = np.frombuffer(M.to_bytes(dval, le), np.uint8).copy()
        dmine, zeros = dev(mine), torch.zeros(count, dtype=torch.int32, device="cuda")
        osh = torch.empty(32 * count, dtype=torch.uint8, device="cuda")
        ost = torch.empty(count, dtype=torch.int32, device="cuda")
        vst = torch.empty(count, dtype=torch.int32, device="cuda")
        sigs, sst = S.sign_batch(name, dh, peer_priv.reshape(-1), dev(nonce.reshape(-1)), le=le)
        dsig = sigs.reshape(-1)
        D.dh_batch(name, dpub, dmine, le=le, priv_idx=zeros, out=(osh, ost))
        E.verify_batch(name, dh, dsig, dpub, le=le, out=vst)
        torch.cuda.synchronize()
        for what, st in (("key_gen", kst), ("sign", sst), ("dh", ost), ("verify", vst)):
            assert not st.any().item(), (name, count, what, st[st != 0][:8].tolist())
        hpub = pub[:4].cpu().numpy()
        for i in range(4):                                 # the first secrets against the plain d Q
            q = bytes(hpub[i])
            R = M.mult(c, dval, (M.num(q[:32], le), M.num(q[32:], le)))
            assert bytes(osh[32 * i:32 * i + 32].cpu().numpy()) == M.to_bytes(R[0], le), (name, count, i)
        ops = (("dh", lambda: D.dh_batch(name, dpub, dmine, le=le, priv_idx=zeros, out=(osh, ost))),
               ("verify", lambda: E.verify_batch(name, dh, dsig, dpub, le=le, out=vst)))
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
        cpu[name] = cpu_rates(name, le, pub.cpu().numpy(), mine)
        print("%-62s reference ecdsa_dh_{be,le} on this box: %s agreements/s" % (name, cpu[name]), flush=True)
res = {"tag": a.tag, "warmup": a.warmup, "rows": rows}
if cpu:
    res["reference_cpu_this_box"] = cpu
else:
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ecdsa_dh.json")))
    res["reference_cpu_other_machine"] = fx["ref_rate"]
    print("reference ecdsa_dh_be, measured on ANOTHER machine (the fixture's generator): %s" % fx["ref_rate"])
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
