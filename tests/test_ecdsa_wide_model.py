"""tests/ecdsa_wide_model.py (the Python-int restatement of the per-item
contract of include/lcb_ecdsa_wide_gpu.h that the GPU tests and tools sign
with) against tests/golden/ecdsa_wide.json, whose statuses the reference
itself returned; and the library's own curve table against the numbers the
reference's loaded curves exported."""
import collections
import errno
import os

import pytest

from tests import ecdsa_wide_model as M

FX = M.load_fixture()
CURVES = M.load_curves(FX)
NAMES = ["secp384r1", "brainpoolP384r1", "brainpoolP512r1", "id-tc26-gost-3410-12-512-paramSetA",
         "id-tc26-gost-3410-12-512-paramSetB", "id-tc26-gost-3410-2012-512-paramSetTest"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_shape():
    golden = os.path.join(ROOT, "tests", "golden")
    largest = max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != "ecdsa_wide.json"
                  and os.path.isfile(os.path.join(golden, f)))
    assert os.path.getsize(M.FIXTURE) <= largest
    assert [c["name"] for c in FX["curves"]] == NAMES
    for i, c in enumerate(FX["curves"]):
        assert c["h"] == 1 and c["algo"] == (M.ALGO_GOST if i >= 3 else M.ALGO_ECDSA)
        assert c["bytes"] == (48 if i < 2 else 64) and all(len(c[k]) == 2 * c["bytes"] for k in M.NUMS)
        assert set(FX["ref_rate"]["per_curve"]) == set(NAMES) and FX["ref_rate"]["per_curve"][c["name"]] > 0
    forms = collections.defaultdict(set)
    for grp in FX["cases"]:
        c = CURVES[grp["curve"]]
        B = c["bytes"]
        forms[grp["curve"]].add(grp["le"])
        names = [k["name"] for k in grp["records"]]
        assert len(names) == len(set(names)) and len(names) >= 40
        st = {k["name"]: k["status"] for k in grp["records"]}
        # what every group must hold, with the status the reference gave
        for name, want in (("valid", 0), ("flip_hash", -2), ("flip_Qy", -1), ("r_eq_n", errno.EINVAL),
                           ("s_eq_n", errno.EINVAL), ("offcurve_and_r_eq_n", -1), ("Qx_eq_p", -1), ("Qy_eq_p", -1),
                           ("hash_zero", 0), ("hash_eq_n", 0), ("hash_ff", 0), ("hash_n_plus_1", 0),
                           ("Q_eq_G", 0), ("Q_eq_minus_G", 0), ("R_at_infinity", -1),
                           ("R_at_infinity_Q_eq_G", -1), ("r_n_minus_1", -2), ("s_n_minus_1", -2)):
            assert st[name] == want, (grp["curve"], name, st[name])
        for hs in (1, 20, B - 1, B, B + 1, 64, 65, 128):
            assert st["hash_size_%d" % hs] == 0
        for hs in (20, B - 1):
            assert st["hash_size_%d_tail_changed" % hs] == 0 and st["hash_size_%d_as_B" % hs] == -2
        for hs in (B + 1, 128):
            assert st["hash_size_%d_as_B" % hs] == 0 and st["hash_size_%d_past_B_changed" % hs] == 0
        assert st["s_zero"] == (errno.EINVAL if c["algo"] == M.ALGO_ECDSA else -2)
        assert st["r_zero"] == -2
        # r = s = 0: no inverse on an ECDSA curve; on a GOST curve u1 = u2 = 0, R at infinity
        assert st["r_s_zero"] == (errno.EINVAL if c["algo"] == M.ALGO_ECDSA else -1)
        # the hash n is not the hash 0: the reference reduces to (e mod (n - 1)) + 1
        assert st["hash_eq_n_sig_of_zero"] == -2
        for k in grp["records"]:
            assert k["le"] == grp["le"] and 1 <= k["hash_size"] <= 128 and len(k["hash"]) >= 2 * k["hash_size"]
            assert all(len(k[f]) == 2 * B for f in ("r", "s", "Qx", "Qy"))
    # le for every GOST curve and one ECDSA curve, be for every ECDSA curve and one GOST curve
    for name, c in CURVES.items():
        assert (c["algo"] == M.ALGO_GOST) in forms[name]
    assert forms["secp384r1"] == {False, True} and forms["id-tc26-gost-3410-12-512-paramSetA"] == {False, True}
    assert sum(len(f) for f in forms.values()) == 8
    # |p - n| is below 2^(4 B + 1) (Hasse), so R.x >= n has a chance below 2^(1 - 4 B): no such valid
    # signature was found
    assert all(not v for note in FX["notes"].values() for v in note.values()) and set(FX["notes"]) == set(NAMES)
    assert not any(k["name"] == "valid_Rx_ge_n" for grp in FX["cases"] for k in grp["records"])
    for c in CURVES.values():
        assert abs(c["p"] - c["n"]) < 1 << (4 * c["bytes"] + 1)
    assert [(g["alg"], g["curve"], g["le"]) for g in FX["messages"]] == [
        ("sha384", "secp384r1", False), ("sha512", "brainpoolP512r1", False),
        ("gost512", "id-tc26-gost-3410-12-512-paramSetA", True)]
    for g in FX["messages"]:
        assert [k["status"] for k in g["records"]] == [0, -2] * 3


def test_all_ones_hash_takes_the_subtractions_the_issue_names():
    """hash_ff reduces by (n - 1) three times on paramSetTest (n = 0x4531...)
    and once on brainpoolP384r1, brainpoolP512r1 and paramSetB."""
    steps = {name: ((1 << (8 * c["bytes"])) - 1) // (c["n"] - 1) for name, c in CURVES.items()}
    assert steps["id-tc26-gost-3410-2012-512-paramSetTest"] == 3
    for name in ("brainpoolP384r1", "brainpoolP512r1", "id-tc26-gost-3410-12-512-paramSetB"):
        assert steps[name] == 1
    assert max(steps.values()) <= 3


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


def test_model_status_of_the_message_records():
    h = lambda s: bytes.fromhex(s)  # noqa: E731
    for g in FX["messages"]:
        c = CURVES[g["curve"]]
        for k in g["records"]:
            hv = h(k["hash"])
            assert M.verify(c, hv, len(hv), h(k["r"]), h(k["s"]), h(k["Qx"]), h(k["Qy"]), g["le"]) == k["status"]


@pytest.mark.parametrize("name", NAMES)
def test_base_point_and_order(name):
    c = CURVES[name]
    top = 8 * c["bytes"] - 2
    assert c["p"] % 2 == 1 and c["n"] % 2 == 1 and c["n"] >> top and c["p"] >> top
    assert M.on_curve(c, c["Gx"], c["Gy"])
    assert M.mult(c, c["n"], M.base(c)) is None
    assert M.mult(c, c["n"] - 1, M.base(c)) == (c["Gx"], c["p"] - c["Gy"])


def test_library_curve_table_equals_reference():
    from liblcb_amd import ecdsa_wide as W
    L = W.ecdsa_wide_lib()
    assert L.lcb_ecdsa_wide_curve_count() == len(FX["curves"]) == len(W.CURVES) == 6
    for i, cj in enumerate(FX["curves"]):
        assert L.lcb_ecdsa_wide_curve_name(i).decode() == cj["name"] == W.CURVES[i]
        assert L.lcb_ecdsa_wide_curve_id(cj["name"].encode()) == i == W.curve_id(cj["name"])
        assert L.lcb_ecdsa_wide_curve_bytes(i) == cj["bytes"] == W.curve_bytes(cj["name"])
        assert W.curve_params(i) == CURVES[cj["name"]], cj["name"]
    assert L.lcb_ecdsa_wide_curve_name(6) is None and L.lcb_ecdsa_wide_curve_name(-1) is None
    assert L.lcb_ecdsa_wide_curve_id(b"secp256r1") == -1 and L.lcb_ecdsa_wide_curve_id(None) == -1
    assert L.lcb_ecdsa_wide_curve_bytes(6) == -1 and L.lcb_ecdsa_wide_curve_bytes(-1) == -1


def test_model_sign_round_trip():
    import random
    rng = random.Random(5)
    for c in CURVES.values():
        B = c["bytes"]
        for le in (False, True):
            d = rng.randrange(1, c["n"])
            Q = M.public_key(c, d)
            h = bytes(rng.randrange(256) for _ in range(B))
            r, s = M.sign(c, h, B, d, rng.randrange(1, 1 << (8 * B)), le)
            args = (M.to_bytes(c, r, le), M.to_bytes(c, s, le), M.to_bytes(c, Q[0], le), M.to_bytes(c, Q[1], le), le)
            assert M.verify(c, h, B, *args) == 0
            assert M.verify(c, bytes([h[0] ^ 1]) + h[1:], B, *args) == -2
