#!/usr/bin/env python3
"""GOST 28147-89 kernel benchmark (include/lcb_gost28147_gpu.h), device
resident: inputs generated on the GPU, HIP-event time per launch, warm-up
excluded, median of --reps launches, the engine clock of the timed launches
themselves (bench.ClockWindow).

Rows: ECB encrypt / decrypt and the MAC over 1M x 1 KiB dense and over 1M
RADIUS-sized ragged packets (20..4096 B back to back).  Reference points in
the same process: the library's ChaCha20 on the same dense layout (the
nearest VALU-bound cipher) and the ECB kernel with its rounds skipped (its
memory ceiling).  Algorithmic bytes: ECB reads and writes every whole block
(+ 12 B of offset and length per ragged buffer); the MAC reads them and
writes 8 B per buffer.  hbm_frac is against 8 TB/s.

usage: python3 tools/gost28147_bench.py [--reps 15] [--warmup 10] [--out profiles/gost28147_bench.json]
       python3 tools/gost28147_bench.py --only ecb_dense --reps 3 --warmup 1   (a counter pass)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liblcb_amd  # noqa: E402
from bench import ClockWindow  # noqa: E402
from liblcb_amd import gost28147 as G  # noqa: E402
from liblcb_amd._lib import F_DEVICE, check, lib  # noqa: E402
from tests.golden_util import packet_layout  # noqa: E402

HBM_BPS = 8e12

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=15)
p.add_argument("--warmup", type=int, default=10)
p.add_argument("--count", type=int, default=1 << 20)
p.add_argument("--len", type=int, default=1024)
p.add_argument("--only", default="", help="comma list of row names")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 1

L = G.gost28147_lib()
s = torch.cuda.current_stream()
key = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(range(32)))
sbox = (ctypes.c_uint8 * 128).from_buffer_copy(G.sbox(G.SBOX_TC26_Z))

dense = liblcb_amd.gen_synthetic(0x6C62636861736821, a.count * a.len)
offs_h, lens_h, ptotal = packet_layout(a.count)
pk = liblcb_amd.gen_synthetic(0x28147, ptotal)
offs = torch.as_tensor(offs_h.astype(np.int64), device="cuda")
lens = torch.as_tensor(lens_h.astype(np.int32), device="cuda")
dst = torch.empty(max(dense.numel(), pk.numel()), dtype=torch.uint8, device="cuda")
macs = torch.empty(a.count * 8, dtype=torch.uint8, device="cuda")
ivs = torch.arange(a.count, dtype=torch.int64, device="cuda").view(torch.uint8)
dense_bytes = a.count * (a.len & ~7)
pk_bytes = int((lens_h.astype(np.int64) & ~7).sum())


def ecb(op, ragged):
    if ragged:
        return lambda: check(L.lcb_gost28147_crypt_batch(op, 0, key, 32, sbox, pk.data_ptr(), dst.data_ptr(),
                                                         offs.data_ptr(), lens.data_ptr(), a.count, 0, 0, F_DEVICE,
                                                         s.cuda_stream))
    return lambda: check(L.lcb_gost28147_crypt_batch(op, 0, key, 32, sbox, dense.data_ptr(), dst.data_ptr(), None,
                                                     None, a.count, a.len, a.len, F_DEVICE, s.cuda_stream))


def mac(ragged):
    if ragged:
        return lambda: check(L.lcb_gost28147_mac_batch(0, key, 32, sbox, pk.data_ptr(), offs.data_ptr(),
                                                       lens.data_ptr(), a.count, 0, 0, macs.data_ptr(), 8, F_DEVICE,
                                                       s.cuda_stream))
    return lambda: check(L.lcb_gost28147_mac_batch(0, key, 32, sbox, dense.data_ptr(), None, None, a.count, a.len,
                                                   a.len, macs.data_ptr(), 8, F_DEVICE, s.cuda_stream))


def copy_only():
    check(L.lcb_gost28147_gpu_copy_probe(dense.data_ptr(), dst.data_ptr(), None, None, a.count, a.len, a.len,
                                         F_DEVICE, s.cuda_stream))


def chacha20():
    check(lib().lcb_chacha_batch(0, key, 32, None, ivs.data_ptr(), 20, dense.data_ptr(), dst.data_ptr(), None, None,
                                 a.count, a.len, a.len, F_DEVICE, s.cuda_stream))


# name, launch, payload bytes, algorithmic bytes moved
ROWS = [
    ("ecb_encrypt_dense", ecb(0, False), dense_bytes, 2 * dense_bytes),
    ("ecb_decrypt_dense", ecb(1, False), dense_bytes, 2 * dense_bytes),
    ("ecb_encrypt_packets", ecb(0, True), pk_bytes, 2 * pk_bytes + 12 * a.count),
    ("ecb_decrypt_packets", ecb(1, True), pk_bytes, 2 * pk_bytes + 12 * a.count),
    ("mac_dense", mac(False), dense_bytes, dense_bytes + 8 * a.count),
    ("mac_packets", mac(True), pk_bytes, pk_bytes + 20 * a.count),
    ("ecb_copy_only_dense", copy_only, dense_bytes, 2 * dense_bytes),
    ("chacha20_dense", chacha20, a.count * a.len, a.count * (2 * a.len + 8)),
]
only = [x for x in a.only.split(",") if x]
rows = {}
for name, launch, payload, moved in ROWS:
    if only and not any(name.startswith(o) for o in only):
        continue
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
    med = ts[len(ts) // 2]
    clock = cw.result(busy_ms=sum(ts))
    rows[name] = {"median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
                  "reps": a.reps, "payload_GiBps": round(payload / (med * 1e-3) / 2**30, 1),
                  "moved_GBps": round(moved / (med * 1e-3) / 1e9, 1),
                  "hbm_frac": round(moved / (med * 1e-3) / HBM_BPS, 4), "clock": clock}
    print("%-22s median %8.4f ms  min %8.4f  %8.1f GiB/s payload  %8.1f GB/s moved  hbm_frac %.3f  clock %s GHz" % (
        name, med, ts[0], rows[name]["payload_GiBps"], rows[name]["moved_GBps"], rows[name]["hbm_frac"],
        clock and clock.get("clock_GHz")), flush=True)
res = {"tag": a.tag, "count": a.count, "len": a.len, "packets": {"bytes": ptotal, "whole_block_bytes": pk_bytes},
       "warmup": a.warmup, "rows": rows}
if "ecb_encrypt_dense" in rows and "chacha20_dense" in rows:
    res["ecb_encrypt_over_chacha20_time"] = round(rows["ecb_encrypt_dense"]["median_ms"] /
                                                  rows["chacha20_dense"]["median_ms"], 3)
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
