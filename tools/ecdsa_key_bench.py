#!/usr/bin/env python3
"""Public-key import / export benchmark (include/lcb_ecdsa_key_gpu.h), device
resident: HIP-event time per launch, warm-up excluded, median of --reps
launches, the engine clock of the timed launches themselves
(bench.ClockWindow).

Rows, per curve (secp256r1, secp256k1 in the be form, CryptoPro-A and
CryptoPro-B in the le form; CryptoPro-B has p = 1 (mod 8), the Tonelli-Shanks
path) and batch size (2^16, 2^20), over keys pub_key_batch made on the device:
  import_compressed   33-byte keys, one size for all
  import_packed       65-byte keys
  import_mixed        33-byte keys, half of them (every second one) with an x
                      whose right-hand side has no root: a refused import
  export_compressed
  verify              verify_batch (liblcb_ecdsa_gpu.so, unchanged) over as
                      many signatures made by sign_batch in the same run: the
                      acceptance number is import_compressed / verify < 1
                      at 2^20 items; the run fails (exit code 1, after the
                      results are written) where it is not
Before any timing every status is checked and the imported keys must equal
the keys they were exported from.

CPU comparison: where oracle/_ref/libref_ecdsa_key.so exists (built by
tests/golden/make_golden_ecdsa_key.py; it travels with the tree) the
reference's own ecdsa_pub_key_import_be / _le is timed on this box over the
first compressed keys with 1 and 16 threads.  Where it does not, the rate the
generator recorded in tests/golden/ecdsa_key.json is printed, labelled as
measured on another machine.

usage: python3 tools/ecdsa_key_bench.py [--reps 11] [--warmup 3] [--out profiles/ecdsa_key_bench.json]
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
from liblcb_amd import ecdsa_key as K  # noqa: E402
from liblcb_amd import ecdsa_sign as S  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=11)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--counts", default="65536,1048576")
p.add_argument("--curves", default="secp256r1,secp256k1,id-gostR3410-2001-CryptoPro-A-ParamSet,"
                                   "id-gostR3410-2001-CryptoPro-B-ParamSet")
p.add_argument("--cpu-items", type=int, default=1024, help="reference calls per thread in the CPU comparison")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 10, "the median of at least 10 repetitions"

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ecdsa_key.so")
s = torch.cuda.current_stream()
dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
KL = K.ecdsa_key_lib()


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


def cpu_rates(name, le, wire):
    """The reference's compressed ecdsa_pub_key_import_be (le: _le) per second on this box, 1 and 16 threads."""
    L = ctypes.CDLL(REF_SO)
    L.ref_key_load.argtypes = [ctypes.c_char_p]
    L.ref_key_import_many.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                      ctypes.c_size_t]
    L.ref_key_import_many.restype = ctypes.c_long
    slot = L.ref_key_load(name.encode())
    assert slot >= 0, name
    n = a.cpu_items
    recs = wire[:n].reshape(-1)
    out = {}
    for threads in (1, 16):
        bufs = [(ctypes.c_uint8 * recs.size).from_buffer_copy(recs.tobytes()) for _ in range(threads)]
        bad = [None] * threads

        def work(t):
            bad[t] = L.ref_key_import_many(slot, int(le), bufs[t], 33, 33, n)

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


def importer(cid, le, keys, size, count, pub, st):
    """One raw import launch into preallocated outputs (no allocation inside the timed region)."""
    return lambda: K.check(KL.lcb_ecdsa_key_import_batch(cid, int(le), keys.data_ptr(), size, None, size, None, count,
                                                         pub.data_ptr(), None, st.data_ptr(), K.F_DEVICE,
                                                         s.cuda_stream))


rows, cpu, ratios = {}, {}, {}
rng = np.random.default_rng(0x6B42)
for name in a.curves.split(","):
    cid = E.curve_id(name)
    le = E.curve_params(name)["algo"] == E.ALGO_GOST      # the natural form of the curve
    for count in [int(x) for x in a.counts.split(",")]:
        seed, nonce, hashes = (rng.integers(0, 256, (count, 32), dtype=np.uint8) for _ in range(3))
        dh = dev(hashes.reshape(-1))
        priv, pub, kst = S.key_gen_batch(name, dev(seed.reshape(-1)), le=le)
        dpub = pub.reshape(-1)
        sigs, sst = S.sign_batch(name, dh, priv.reshape(-1), dev(nonce.reshape(-1)), le=le)
        dsig = sigs.reshape(-1)
        vst = torch.empty(count, dtype=torch.int32, device="cuda")
        comp, csz, cst = K.export_batch(name, dpub, form=K.COMPRESSED, le=le)
        pack, psz, pst = K.export_batch(name, dpub, form=K.PACKED, le=le)
        # keys without a root into every second slot: random x, drawn again where the import accepted it
        mixed = comp.clone()
        todo = torch.arange(count, device="cuda") % 2 == 1
        odd = todo.clone()
        for _ in range(64):
            if not todo.any().item():
                break
            cand = mixed.clone()
            cand[:, 1:] = dev(rng.integers(0, 256, (count, 32), dtype=np.uint8))
            cand[:, 32 if le else 1] &= 0x3F               # below every p of the table
            _, nst, _ = K.import_batch(name, cand, le=le)
            take = todo & (nst != 0)
            mixed[take] = cand[take]
            todo &= ~take
        assert not todo.any().item(), (name, count, "no non-residue found for some slot")
        opub = torch.empty(64 * count, dtype=torch.uint8, device="cuda")
        ost = torch.empty(count, dtype=torch.int32, device="cuda")
        osz = torch.empty(count, dtype=torch.int32, device="cuda")
        oform = torch.empty(33 * count, dtype=torch.uint8, device="cuda")
        imp_c = importer(cid, le, comp, 33, count, opub, ost)
        imp_p = importer(cid, le, pack, 65, count, opub, ost)
        imp_m = importer(cid, le, mixed, 33, count, opub, ost)
        exp_c = lambda: K.check(KL.lcb_ecdsa_key_export_batch(  # noqa: E731
            cid, int(le), K.COMPRESSED, dpub.data_ptr(), None, count, oform.data_ptr(), 33, osz.data_ptr(),
            ost.data_ptr(), K.F_DEVICE, s.cuda_stream))
        ver = lambda: E.verify_batch(name, dh, dsig, dpub, le=le, out=vst)  # noqa: E731
        # statuses and bytes before any timing
        for what, st in (("key_gen", kst), ("sign", sst), ("export", cst), ("export", pst)):
            assert not st.any().item(), (name, count, what)
        for what, launch in (("compressed", imp_c), ("packed", imp_p)):
            launch()
            torch.cuda.synchronize()
            assert not ost.any().item() and torch.equal(opub, dpub), (name, count, what)
        imp_m()
        ver()
        torch.cuda.synchronize()
        refused = int((ost != 0).sum().item())
        assert torch.equal(ost != 0, odd) and refused == count // 2, (name, count, refused)
        assert not vst.any().item(), (name, count, "verify")
        med_of = {}
        for op, launch in (("import_compressed", imp_c), ("import_packed", imp_p), ("import_mixed", imp_m),
                           ("export_compressed", exp_c), ("verify", ver)):
            ts, clock = timed(launch)
            med = med_of[op] = ts[len(ts) // 2]
            row = "%s_%s_%d" % (name, op, count)
            rows[row] = {"median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
                         "reps": a.reps, "items_per_s": round(count / (med * 1e-3)), "clock": clock}
            if op == "import_mixed":
                rows[row]["refused"] = refused
            print("%-72s median %9.4f ms  min %9.4f  %12d items/s  clock %s GHz" % (
                row, med, ts[0], rows[row]["items_per_s"], clock and clock.get("clock_GHz")), flush=True)
        ratios["%s_%d" % (name, count)] = round(med_of["import_compressed"] / med_of["verify"], 4)
        print("%-72s import_compressed / verify = %.4f" % ("%s_%d" % (name, count), ratios["%s_%d" % (name, count)]),
              flush=True)
    if os.path.exists(REF_SO):
        cpu[name] = cpu_rates(name, le, comp.cpu().numpy())
        print("%-72s reference ecdsa_pub_key_import_{be,le} on this box: %s keys/s" % (name, cpu[name]), flush=True)
res = {"tag": a.tag, "warmup": a.warmup, "rows": rows, "import_compressed_over_verify": ratios}
if cpu:
    res["reference_cpu_this_box"] = cpu
else:
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ecdsa_key.json")))
    res["reference_cpu_other_machine"] = fx["ref_rate"]
    print("reference ecdsa_pub_key_import_be, measured on ANOTHER machine (the fixture's generator): %s"
          % fx["ref_rate"])
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
# Acceptance: importing on the device must cost less device time than verifying, or it would not relieve the verifier.
slow = {k: v for k, v in ratios.items() if int(k.rsplit("_", 1)[1]) >= 1 << 20 and v >= 1.0}
if slow:
    raise SystemExit("FAIL: compressed import is not faster than verify_batch at 2^20 items: %s" % slow)
