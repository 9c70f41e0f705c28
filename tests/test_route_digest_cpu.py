"""What ``train_ddp.Solver`` routes every config's model to under every routing switch, against tests/golden/route_digest.json (written
by tests/golden/make_route_digest.py at the commit whose routing is the reference): per module its class and its ``_ssdk_*`` /
``native_*`` attributes, and ``headconv.WGRAD_MIN_PIXELS`` (tests/routedigest.py).  No device is needed: the Solver routes the model
on the CPU.  The conditions on the golden file below are conditions, not measurements: they keep the digest from going blind."""
import json
import os

import pytest

import routedigest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_digest.json")
# the values that are not what an unset variable means (SSDK_DENSE3_TRAIN: unset depends on the model, so both)
NON_DEFAULT = [(name, v) for name, (values, default) in routedigest.SWITCHES.items() for v in values if v != default]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _differs(golden, setting):
    """The configs whose digest under ``setting`` is not the one with nothing set."""
    return [c for c in routedigest.configs() if golden["%s/%s" % (c, setting)] != golden[c + "/unset"]]


def test_golden_names_every_config_under_every_setting(golden):
    assert len(routedigest.configs()) >= 18 and len(routedigest.SETTINGS) == 1 + 2 * 15 + 3 + 3
    assert list(golden) == routedigest.keys()  # a new config without golden entries fails here


@pytest.mark.parametrize("switch,value", NON_DEFAULT)
def test_every_switch_moves_the_digest_of_some_config(golden, switch, value):
    """When the golden file was written: FAST_BN=0 18 configs, FUSE_BN_ACT=0 18, BN_DEFER=0 2, BN_STATS_FUSED=0 14, SHUFFLE_TRAIN=0 2,
    DENSE_TRAIN=1 2, PW_GEMM=0 18, GCONV_TRAIN=0 3, STEM7_TRAIN=1 9, MBCONV_TRAIN=0 1, HEAD_PAIR=0 3, DENSE3_TRAIN=0 7, DENSE3_TRAIN=1 7,
    NECK_TRAIN=0 11, CAT_TRAIN=0 6, CONVT_TRAIN=1 2, CONV3_NATIVE=0 18, CONV3_NATIVE=1 11."""
    assert len(NON_DEFAULT) == 14 + 2 + 2
    assert len(_differs(golden, "%s=%s" % (switch, value))) >= 1


def test_the_default_set_explicitly_is_unset(golden):
    for switch, (_, default) in routedigest.SWITCHES.items():
        if default is not None:
            assert _differs(golden, "%s=%s" % (switch, default)) == [], switch
    # SSDK_DENSE3_TRAIN: what unset means depends on the model, so each value moves some configs and no config moves under both
    off, on = _differs(golden, "SSDK_DENSE3_TRAIN=0"), _differs(golden, "SSDK_DENSE3_TRAIN=1")
    assert off and on and not set(off) & set(on)


def test_sync_bn_moves_every_config(golden):
    for setting in ("sync_bn", "sync_bn,SSDK_FAST_BN=0", "sync_bn,SSDK_DENSE_TRAIN=1"):
        assert _differs(golden, setting) == routedigest.configs(), setting


@pytest.mark.parametrize("cfg_name", routedigest.configs())
def test_routing_is_what_the_reference_commit_routed(cfg_name, golden):
    wrong = [s for s in routedigest.SETTINGS if routedigest.digest(routedigest.canonical(cfg_name, s)) != golden["%s/%s" % (cfg_name, s)]]
    assert wrong == [], "print the text of a key on both commits and diff: python tests/routedigest.py %s/%s" % (cfg_name, wrong[0])
