#!/usr/bin/env python3
"""Streaming-digest update benchmark (include/lcb_hash_stream_gpu.h), device
resident: inputs generated on the GPU, HIP-event time per launch, warm-up
excluded, median of --reps launches, the engine clock of the timed launches
themselves (bench.ClockWindow).

Rows: lcb_hash_stream_update for MD5, SHA-256 and GOST-256 at 65,536 streams
x {256 B, 1 KiB, 4 KiB} dense chunks (stream i takes chunk i, no index list:
the call waits for nothing), and in the same run lcb_hash_batch over the same
bytes as the yardstick (one-shot digests: it also pads and writes digests,
the update writes its contexts back).  Every timed update continues the
streams the previous one left, so the contexts are read and written each
time.  ratio = update GiB/s over lcb_hash_batch GiB/s.

usage: python3 tools/stream_bench.py [--reps 200] [--warmup 20] [--out profiles/stream_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liblcb_amd  # noqa: E402
from bench import ClockWindow  # noqa: E402
from liblcb_amd import stream as S  # noqa: E402
from liblcb_amd._lib import F_DEVICE, check, lib  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=200)
p.add_argument("--warmup", type=int, default=20)
p.add_argument("--streams", type=int, default=65536)
p.add_argument("--lens", default="256,1024,4096")
p.add_argument("--algs", default="md5,sha256,gost256")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 1

SL, HL = S.stream_lib(), lib()
s = torch.cuda.current_stream()
lens = [int(x) for x in a.lens.split(",")]
data = liblcb_amd.gen_synthetic(0x6C62636861736821, a.streams * max(lens))
dig = torch.empty(a.streams * 64, dtype=torch.uint8, device="cuda")


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


rows = {}
for name in a.algs.split(","):
    alg = liblcb_amd.ALG_IDS[name]
    st = S.StreamSet(alg, a.streams)
    for n in lens:
        payload = a.streams * n
        for kind, launch in (
                ("update", lambda: check(SL.lcb_hash_stream_update(st._h, None, data.data_ptr(), None, None, a.streams,
                                                                   n, n, F_DEVICE, s.cuda_stream))),
                ("batch", lambda: check(HL.lcb_hash_batch(alg, None, 0, data.data_ptr(), None, None, a.streams, n, n,
                                                          dig.data_ptr(), F_DEVICE, s.cuda_stream)))):
            ts, clock = timed(launch)
            med = ts[len(ts) // 2]
            rows["%s_%s_%d" % (name, kind, n)] = {
                "median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "reps": a.reps,
                "GiBps": round(payload / (med * 1e-3) / 2**30, 1), "clock": clock}
            print("%-24s median %8.4f ms  min %8.4f  %8.1f GiB/s  clock %s GHz" % (
                "%s_%s_%d" % (name, kind, n), med, ts[0], rows["%s_%s_%d" % (name, kind, n)]["GiBps"],
                clock and clock.get("clock_GHz")), flush=True)
        u, b = rows["%s_update_%d" % (name, n)], rows["%s_batch_%d" % (name, n)]
        u["ratio_to_lcb_hash_batch"] = round(u["GiBps"] / b["GiBps"], 3) if b["GiBps"] else None
    st.close()
res = {"tag": a.tag, "streams": a.streams, "lens": lens, "warmup": a.warmup, "rows": rows}
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
