"""Reader of tests/golden/ecdsa_key.json (the reference's public-key import
and export cases, tests/golden/make_golden_ecdsa_key.py) for the tests of
liblcb_ecdsa_key_gpu.so: the rows as dicts with their byte strings put
together from the group's table of numbers."""
import json
import os

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecdsa_key.json")
ZERO64 = bytes(64)


def pieces(g, p):
    """The byte string a list of pieces stands for: a string is hex, an int i is nums[i]."""
    return b"".join(bytes.fromhex(q) if isinstance(q, str) else bytes.fromhex(g["nums"][q]) for q in p)


def load():
    """{source, ref_rate, groups: [{curve, le, imports, exports}]}.

    imports  {name, key, key_y (None: NULL), status, infinity, xy (64 bytes, zeros unless accepted and finite)}
    exports  {name, compress, infinity, xy (64 bytes), out}
    """
    with open(PATH) as f:
        fx = json.load(f)
    assert fx["import_columns"] == ["name", "key", "key_y", "status", "infinity", "xy"]
    assert fx["export_columns"] == ["name", "compress", "infinity", "xy", "out"]
    groups = []
    for g in fx["groups"]:
        imports = [{"name": r[0], "key": pieces(g, r[1]), "key_y": None if r[2] is None else pieces(g, r[2]),
                    "status": r[3], "infinity": r[4], "xy": pieces(g, r[5]) or ZERO64} for r in g["import"]]
        exports = [{"name": r[0], "compress": r[1], "infinity": r[2], "xy": pieces(g, r[3]), "out": pieces(g, r[4])}
                   for r in g["export"]]
        groups.append({"curve": g["curve"], "le": bool(g["le"]), "imports": imports, "exports": exports})
    return {"source": fx["source"], "ref_rate": fx["ref_rate"], "groups": groups}


def flip_key(key):
    """The same key in the other byte order: the prefix byte of the 33- and
    65-byte forms stays first, every 32-byte number after it is reversed.
    Other sizes have no numbers in them the import would read."""
    n = len(key)
    if n in (32, 64):
        return b"".join(key[i:i + 32][::-1] for i in range(0, n, 32))
    if n in (33, 65):
        return key[:1] + b"".join(key[i:i + 32][::-1] for i in range(1, n, 32))
    return key


def flip_xy(xy):
    return xy[:32][::-1] + xy[32:][::-1]
