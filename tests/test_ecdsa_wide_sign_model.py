"""tests/golden/ecdsa_wide_sign.json against the Python-int model and against
the library's curve table, without a GPU: the model (tests/ecdsa_wide_model.sign,
tests/ecdsa_wide_sign_cases.key_gen / pub_key) reproduces every status and
every byte the reference returned, and the curves the fixture was generated
over are those lcb_ecdsa_wide_curve_params reports."""
import pytest

from liblcb_amd import ecdsa_wide
from tests import ecdsa_wide_model as M
from tests import ecdsa_wide_sign_cases as K

FX = K.load_fixture()
CURVES = M.load_curves()
IDS = ["%s-%s" % (g["curve"], "le" if g["le"] else "be") for g in FX["groups"]]


@pytest.mark.parametrize("g", FX["groups"], ids=IDS)
def test_model_reproduces_every_record(g):
    c, le = CURVES[g["curve"]], g["le"]
    hx = lambda t: tuple(v.hex() if isinstance(v, bytes) else v for v in t)  # noqa: E731
    bad = []
    for k in g["sign"]:
        got = hx(K.sign(c, bytes.fromhex(k["hash"]), k["hash_size"], bytes.fromhex(k["d"]), bytes.fromhex(k["rnd"]),
                        le))
        if got != (k["status"], k["r"], k["s"]):
            bad.append(("sign", k["name"]))
    for k in g["key_gen"]:
        if hx(K.key_gen(c, bytes.fromhex(k["rnd"]), le)) != (k["status"], k["d"], k["Qx"], k["Qy"]):
            bad.append(("key_gen", k["name"]))
    for k in g["pub_key"]:
        if hx(K.pub_key(c, bytes.fromhex(k["d"]), le)) != (k["status"], k["Qx"], k["Qy"]):
            bad.append(("pub_key", k["name"]))
    assert not bad, bad


def test_status_0_signatures_verify_in_the_model():
    """Every fourth record (the host program of test_ecdsa_wide_sign_host.py
    verifies all of them); the first one moves with the group, so every
    position of the case list is met in one group or another."""
    n = 0
    for gi, g in enumerate(FX["groups"]):
        c, le = CURVES[g["curve"]], g["le"]
        for k in g["sign"][gi % 4::4]:
            if k["status"] == 0 and int(k["d"], 16) != 0:
                _, qx, qy = K.pub_key(c, bytes.fromhex(k["d"]), le)
                assert M.verify(c, bytes.fromhex(k["hash"]), k["hash_size"], bytes.fromhex(k["r"]),
                                bytes.fromhex(k["s"]), qx, qy, le) == 0, (g["curve"], k["name"])
                n += 1
    assert n > 40


def test_fixture_curves_are_the_library_table():
    assert {g["curve"] for g in FX["groups"]} == set(ecdsa_wide.CURVES)
    for cid, name in enumerate(ecdsa_wide.CURVES):
        got = ecdsa_wide.curve_params(cid)
        want = CURVES[name]
        assert got["name"] == name
        for k in M.NUMS + ("algo", "h", "bytes"):
            assert got[k] == want[k], (name, k)
