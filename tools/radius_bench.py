#!/usr/bin/env python3
"""Batched RADIUS sign / verify benchmark (include/lcb_radius_gpu.h), device
resident: packets built on the GPU, HIP-event time per call, warm-up excluded,
median of --reps calls, the engine clock of the timed calls themselves
(bench.ClockWindow).

Packets: --count (1M) packed back to back, buffer lengths 20..4096 from mix64
as the packet rows of bench.py (tests/golden_util.packet_layout), 64 secrets
(packet_keys / packet_key_index).  Each holds a valid attribute list:
Vendor-Specific attributes of 255 bytes and one shorter fill the packet (a
buffer whose fill would leave one byte keeps it as a tail past Length); codes
Access-Request / Accounting-Request / Access-Accept 2:1:1; a
zero authenticator in the Accounting-Requests; a
Message-Authenticator in --ma-share of the packets that have room, a
User-Password of 1..8 blocks in --pw-share of the Access-Requests that have
room.  Replies carry their request's authenticator (req_hdrs).

Rows, one JSON line each: sign, then verify of what sign left (every call
starts from the same bytes: a device copy ahead of the timed span), with
packets/s, GiB/s over the sum of Length, that over the 8 TB/s peak, and the
clock; errors must be all 0 and verify must give the unsigned packets'
User-Passwords back.  Then the three bare keyed MD5 passes this layer sits on,
over the same packets, keys and key indices: HMAC and H(m || K) over
[0, Length), H(K || m) over every packet's 16-byte authenticator; the same
device copy runs ahead of each of their timed calls, so every row has the same
duty cycle (the clock of a row follows how busy the chip is).  With
--host-layer N: liblcb_amd.radius.radius_pkt_verify_batch(device=True), the
per-packet host layer, and verify_packed on the first N packets (wall time).

usage: python3 tools/radius_bench.py [--reps 9] [--warmup 3] [--host-layer 65536] [--out profiles/radius_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liblcb_amd  # noqa: E402
from bench import ClockWindow  # noqa: E402
from liblcb_amd import radius_batch as RB  # noqa: E402
from liblcb_amd._lib import F_DEVICE, check, lib  # noqa: E402
from tests.golden_util import packet_key_index, packet_keys, packet_layout  # noqa: E402

HBM_BPS = 8e12

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=9)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--count", type=int, default=1 << 20)
p.add_argument("--ma-share", type=float, default=0.5)
p.add_argument("--pw-share", type=float, default=0.5)
p.add_argument("--host-layer", type=int, default=0, help="also time the per-packet host layer on the first N packets")
p.add_argument("--tag", default="")
p.add_argument("--out", default="")
a = p.parse_args()
assert a.reps >= 1

s = torch.cuda.current_stream()
dev = lambda x: torch.as_tensor(x, device="cuda")  # noqa: E731

# ------------------------------------------------------------- the packets
n = a.count
offs_h, bufs_h, total = packet_layout(n)
keys = [bytes(k) for k in packet_keys()]
kidx_h = packet_key_index(n)
rng = np.random.default_rng(0x52414449)
B = bufs_h.astype(np.int64)
code = rng.choice(np.array([1, 4, 2], np.int64), n, p=[0.5, 0.25, 0.25])
has_ma = (rng.random(n) < a.ma_share) & (B >= 38)
pwb = np.where((code == 1) & (rng.random(n) < a.pw_share), 1 + rng.integers(0, 8, n), 0)
pwb = np.where(B >= 20 + 18 * has_ma + 2 + 16 * pwb, pwb, 0)
pos0 = 20 + 18 * has_ma + np.where(pwb > 0, 2 + 16 * pwb, 0)
rem = B - pos0
rem -= (rem % 255 == 1)                      # one byte cannot hold an attribute: it stays a tail past Length
length = pos0 + rem
req_auth = rng.integers(0, 256, (n, 16), dtype=np.uint8)
req_hdrs_h = np.zeros((n, 20), np.uint8)
req_hdrs_h[code == 2, 0] = 1                 # the replies answer an Access-Request
req_hdrs_h[:, 4:] = req_auth
req_hdrs_h[code != 2] = 0

blob = liblcb_amd.gen_synthetic(0x5241444955, total)
o = dev(offs_h.astype(np.int64))


def put(at, val, mask=None):
    """blob[o + at] = val for the packets of mask (at, val: per-packet arrays or scalars)."""
    idx = o + dev(np.broadcast_to(np.asarray(at, np.int64), (n,)).copy())
    v = dev(np.broadcast_to(np.asarray(val, np.int64), (n,)).astype(np.uint8))
    if mask is not None:
        m = dev(mask)
        idx, v = idx[m], v[m]
    blob[idx] = v


put(0, code)
put(2, length >> 8)
put(3, length & 255)
put(20, 80, has_ma)
put(21, 18, has_ma)
put(20 + 18 * has_ma, 2, pwb > 0)
put(21 + 18 * has_ma, 2 + 16 * pwb, pwb > 0)
for j in range(16):
    put(4 + j, req_auth[:, j], code == 2)    # a reply is signed with its request's authenticator inside
    put(4 + j, 0, code == 4)                 # an Accounting-Request with zeros (radius_pkt_init, radius.h:1442-1447)
for j in range(17):                          # Vendor-Specific attributes fill the rest
    left = rem - 255 * j
    put(pos0 + 255 * j, 26, left > 0)
    put(pos0 + 255 * j + 1, np.minimum(left, 255), left > 0)
torch.cuda.synchronize()

bufs = dev(bufs_h.astype(np.int32))
lens = dev(length.astype(np.int32))
kidx = dev(kidx_h.astype(np.int32))
req_hdrs = dev(req_hdrs_h.reshape(-1))
pre = blob.clone()
sum_len = int(length.sum())
share = {"packets": n, "buffer_bytes": total, "sum_length": sum_len, "keys": len(keys),
         "codes": {"access_request": int((code == 1).sum()), "accounting_request": int((code == 4).sum()),
                   "access_accept": int((code == 2).sum())},
         "msg_authenticator": int(has_ma.sum()), "user_password": int((pwb > 0).sum()),
         "password_blocks": int(pwb.sum()), "tails_past_length": int((B != length).sum()),
         "ma_share": a.ma_share, "pw_share": a.pw_share}
print(json.dumps({"row": "packets", **share}), flush=True)


def timed(name, launch, reset=None, payload=sum_len, extra=None):
    for _ in range(a.warmup):
        if reset is not None:
            reset()
        launch()
    torch.cuda.synchronize()
    cw = ClockWindow(s)
    cw.begin()
    evs = []
    for _ in range(a.reps):
        if reset is not None:
            reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        launch()
        e1.record(s)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    cw.end()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    med = ts[len(ts) // 2]
    row = {"row": name, "median_ms": round(med, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
           "reps": a.reps, "packets_per_s": round(n / (med * 1e-3)), "GiB_s": round(payload / (med * 1e-3) / 2**30, 2),
           "hbm_frac": round(payload / (med * 1e-3) / HBM_BPS, 4), "clock": cw.result(busy_ms=sum(ts))}
    row.update(extra() if extra else {})
    print(json.dumps(row), flush=True)
    return row


rows = {"packets": share}


# The C ABI itself (the Python wrapper's extent check synchronises the stream).
RL = RB.radius_lib()
kblob = np.frombuffer(b"".join(keys), np.uint8)
klen = np.array([len(k) for k in keys], np.uint32)
koff = np.zeros(len(keys), np.uint64)
koff[1:] = np.cumsum(klen[:-1], dtype=np.uint64)
err = torch.empty(n, dtype=torch.int32, device="cuda")
KT = (kblob.ctypes.data, koff.ctypes.data, klen.ctypes.data, len(keys))


def do_sign():
    check(RL.radius_pkt_sign_batch(blob.data_ptr(), o.data_ptr(), bufs.data_ptr(), n, 0, 0, *KT, kidx.data_ptr(),
                                   err.data_ptr(), F_DEVICE, s.cuda_stream))


def do_verify():
    check(RL.radius_pkt_verify_batch(blob.data_ptr(), o.data_ptr(), bufs.data_ptr(), n, 0, 0, *KT, kidx.data_ptr(),
                                     req_hdrs.data_ptr(), err.data_ptr(), F_DEVICE, s.cuda_stream))


rows["sign"] = timed("sign", do_sign, reset=lambda: blob.copy_(pre),
                     extra=lambda: {"errors_nonzero": int((err != 0).sum().item())})
signed = blob.clone()
rows["verify"] = timed("verify", do_verify, reset=lambda: blob.copy_(signed),
                       extra=lambda: {"errors_nonzero": int((err != 0).sum().item())})
# verify gives back what sign took: every byte but the fields sign wrote (the authenticator, the
# Message-Authenticator's data) equals the unsigned packet, decoded User-Passwords included
allowed = torch.zeros(total, dtype=torch.bool, device="cuda")
ma_o = o[dev(has_ma)]
for j in range(16):
    allowed[o + 4 + j] = True
    allowed[ma_o + 22 + j] = True
ok = True
for c in range(0, total, 1 << 28):
    e = min(total, c + (1 << 28))
    ok = ok and not bool(((blob[c:e] != pre[c:e]) & ~allowed[c:e]).any().item())
rows["verify"]["roundtrip_ok"] = ok
del allowed
print(json.dumps({"row": "roundtrip", "passwords_restored_and_only_signed_fields_differ": ok}), flush=True)

# ------------------------------------------ the three bare keyed MD5 passes
dig = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
o4 = o + 4


def keyed(mode, offsets, lengths, fixed):
    return lambda: check(lib().lcb_hash_batch_keyed(1, mode, kblob.ctypes.data, koff.ctypes.data, klen.ctypes.data,
                                                    len(keys), kidx.data_ptr(), blob.data_ptr(), offsets.data_ptr(),
                                                    lengths.data_ptr() if lengths is not None else None, n, 0, fixed,
                                                    dig.data_ptr(), F_DEVICE, s.cuda_stream))


# the same device copy ahead of every timed call as in the sign / verify rows: one duty cycle for all rows
again = lambda: blob.copy_(signed)  # noqa: E731
rows["keyed_hmac"] = timed("keyed_hmac", keyed(1, o, lens, 0), reset=again)
rows["keyed_suffix"] = timed("keyed_suffix", keyed(3, o, lens, 0), reset=again)
rows["keyed_prefix_16"] = timed("keyed_prefix_16", keyed(2, o4, None, 16), reset=again, payload=16 * n)
floor = sum(rows[k]["median_ms"] for k in ("keyed_hmac", "keyed_suffix", "keyed_prefix_16"))
res = {"tag": a.tag, "warmup": a.warmup, "rows": rows, "bare_three_passes_ms": round(floor, 4),
       "sign_over_bare": round(rows["sign"]["median_ms"] / floor, 3),
       "verify_over_bare": round(rows["verify"]["median_ms"] / floor, 3)}

# ------------------------------------ the per-packet host layer, before/after
if a.host_layer:
    from liblcb_amd.radius import radius_pkt_verify_batch
    m = min(a.host_layer, n)
    end = int(offs_h[m - 1]) + int(bufs_h[m - 1])
    host = signed[:end].cpu().numpy()
    pk = [bytes(host[int(x):int(x) + int(b)]) for x, b in zip(offs_h[:m], bufs_h[:m])]
    reqs = [bytes(r) if r[0] else None for r in req_hdrs_h[:m]]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e_old, _ = radius_pkt_verify_batch(pk, keys, kidx_h[:m], reqs, device=True)
    torch.cuda.synchronize()
    t_old = time.perf_counter() - t0
    sub = signed[:end].clone()
    ts = []
    for _ in range(3):
        sub.copy_(signed[:end])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e_new = RB.verify_packed(sub, keys, kidx[:m].contiguous(), o[:m].contiguous(), bufs[:m].contiguous(),
                                 req_hdrs=req_hdrs[:20 * m].contiguous())
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    res["host_layer"] = {"packets": m, "radius_pkt_verify_batch_device_ms": round(t_old * 1e3, 2),
                         "verify_packed_wall_ms": round(sorted(ts)[1] * 1e3, 3),
                         "errors_equal": bool(np.array_equal(e_old, e_new.cpu().numpy())),
                         "speedup": round(t_old / sorted(ts)[1], 1)}
    print(json.dumps({"row": "host_layer", **res["host_layer"]}), flush=True)

if a.out:
    rows = res.pop("rows")                   # one row per line
    with open(a.out, "w") as f:
        f.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in res.items()))
        f.write(' "rows": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items()))
        f.write("\n }\n}\n")
    res["rows"] = rows
print(json.dumps(res))
