"""tests/ecdsa_model.py (the Python-int restatement of the per-item contract
of include/lcb_ecdsa_gpu.h that the GPU tests and tools sign with) against
tests/golden/ecdsa.json, whose statuses the reference itself returned; and
the library's own curve table against the numbers the reference's loaded
curves exported."""
import collections
import errno
import os

import pytest

from tests import ecdsa_model as M

FX = M.load_fixture()
CURVES = M.load_curves(FX)
GOST_NAMES = ["id-GostR3410-2001-ParamSet-cc", "id-gostR3410-2001-Test_ParamSet"] + [
    "id-gostR3410-2001-CryptoPro-%s-ParamSet" % s for s in ("A", "B", "C", "XchA", "XchB")]


def test_fixture_shape():
    assert os.path.getsize(M.FIXTURE) < 250 * 1024
    assert [c["name"] for c in FX["curves"]] == ["secp256k1", "secp256r1", "brainpoolP256r1"] + GOST_NAMES
    for c in FX["curves"]:
        assert c["h"] == 1 and c["algo"] == (M.ALGO_GOST if c["name"] in GOST_NAMES else M.ALGO_ECDSA)
    forms = collections.defaultdict(set)
    for grp in FX["cases"]:
        forms[grp["curve"]].add(grp["le"])
        names = [k["name"] for k in grp["records"]]
        assert len(names) == len(set(names)) and len(names) >= 24
        st = {k["name"]: k["status"] for k in grp["records"]}
        # what every group must hold, with the status the reference gave
        for name, want in (("valid", 0), ("flip_hash", -2), ("flip_Qy", -1), ("r_eq_n", errno.EINVAL),
                           ("s_eq_n", errno.EINVAL), ("offcurve_and_r_eq_n", -1), ("Qx_eq_p", -1),
                           ("hash_zero", 0), ("hash_eq_n", 0), ("hash_ff", 0), ("hash_size_20", 0),
                           ("hash_size_64", 0), ("Q_eq_G", 0), ("Q_eq_minus_G", 0), ("R_at_infinity", -1),
                           ("R_at_infinity_Q_eq_G", -1), ("r_n_minus_1", -2), ("s_n_minus_1", -2)):
            assert st[name] == want, (grp["curve"], name, st[name])
        algo = CURVES[grp["curve"]]["algo"]
        assert st["s_zero"] == (errno.EINVAL if algo == M.ALGO_ECDSA else -2)
        assert st["r_zero"] == -2
        # the hash n is not the hash 0: the reference reduces to (e mod (n - 1)) + 1
        assert st["hash_eq_n_sig_of_zero"] == -2
        for k in grp["records"]:
            assert k["le"] == grp["le"] and 1 <= k["hash_size"] <= 64 and len(k["hash"]) >= 2 * k["hash_size"]
    # le for every GOST curve and one ECDSA curve, be for every ECDSA curve and one GOST curve
    for name, c in CURVES.items():
        assert (c["algo"] == M.ALGO_GOST) in forms[name]
    assert sum(1 for n, f in forms.items() if CURVES[n]["algo"] == M.ALGO_ECDSA and True in f) == 1
    assert sum(1 for n, f in forms.items() if CURVES[n]["algo"] == M.ALGO_GOST and False in f) == 1
    # a valid signature whose R.x is >= n exists where p is far above n
    assert any(k["name"] == "valid_Rx_ge_n" for grp in FX["cases"] for k in grp["records"]
               if grp["curve"] == "id-GostR3410-2001-ParamSet-cc")


@pytest.mark.parametrize("grp", FX["cases"], ids=lambda g: "%s-%s" % (g["curve"], "le" if g["le"] else "be"))
def test_model_status_equals_reference(grp):
    c = CURVES[grp["curve"]]
    h = lambda s: bytes.fromhex(s)  # noqa: E731
    bad = []
    for k in grp["records"]:
        got = M.verify(c, h(k["hash"]), k["hash_size"], h(k["r"]), h(k["s"]), h(k["Qx"]), h(k["Qy"]), k["le"])
        if got != k["status"]:
            bad.append((k["name"], got, k["status"]))
    assert not bad, bad


def test_valid_Rx_ge_n_case_needs_the_reduction():
    for grp in FX["cases"]:
        c = CURVES[grp["curve"]]
        for k in grp["records"]:
            if k["name"] != "valid_Rx_ge_n":
                continue
            # recompute R as the verifier does and look at its x
            le = k["le"]
            e = M.hash_number(c, bytes.fromhex(k["hash"]), k["hash_size"], le)
            r, s = M.num(bytes.fromhex(k["r"]), le), M.num(bytes.fromhex(k["s"]), le)
            Q = (M.num(bytes.fromhex(k["Qx"]), le), M.num(bytes.fromhex(k["Qy"]), le))
            n = c["n"]
            if c["algo"] == M.ALGO_ECDSA:
                w = pow(s, -1, n)
                u1, u2 = e * w % n, r * w % n
            else:
                w = pow(e or 1, -1, n)
                u1, u2 = s * w % n, (n - w) * r % n
            R = M.add(c, M.mult(c, u1, M.base(c)), M.mult(c, u2, Q))
            assert R[0] >= n and R[0] % n == r


@pytest.mark.parametrize("name", list(CURVES))
def test_base_point_and_order(name):
    c = CURVES[name]
    assert c["p"] % 2 == 1 and c["n"] % 2 == 1 and c["n"] >> 254 and c["p"] >> 254
    assert M.on_curve(c, c["Gx"], c["Gy"])
    assert M.mult(c, c["n"], M.base(c)) is None
    assert M.mult(c, c["n"] - 1, M.base(c)) == (c["Gx"], c["p"] - c["Gy"])


def test_library_curve_table_equals_reference():
    from liblcb_amd import ecdsa as E
    L = E.ecdsa_lib()
    assert L.lcb_ecdsa_curve_count() == len(FX["curves"]) == len(E.CURVES) == 10
    for i, cj in enumerate(FX["curves"]):
        assert L.lcb_ecdsa_curve_name(i).decode() == cj["name"] == E.CURVES[i]
        assert L.lcb_ecdsa_curve_id(cj["name"].encode()) == i == E.curve_id(cj["name"])
        got = E.curve_params(i)
        assert got == CURVES[cj["name"]], cj["name"]
    assert L.lcb_ecdsa_curve_name(10) is None and L.lcb_ecdsa_curve_name(-1) is None
    assert L.lcb_ecdsa_curve_id(b"secp384r1") == -1 and L.lcb_ecdsa_curve_id(None) == -1


def test_model_sign_round_trip():
    import random
    rng = random.Random(5)
    for c in CURVES.values():
        for le in (False, True):
            d = rng.randrange(1, c["n"])
            Q = M.public_key(c, d)
            h = bytes(rng.randrange(256) for _ in range(32))
            r, s = M.sign(c, h, 32, d, rng.randrange(1, 1 << 256), le)
            args = (M.to_bytes(r, le), M.to_bytes(s, le), M.to_bytes(Q[0], le), M.to_bytes(Q[1], le), le)
            assert M.verify(c, h, 32, *args) == 0
            assert M.verify(c, bytes([h[0] ^ 1]) + h[1:], 32, *args) == -2
