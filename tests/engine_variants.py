"""The engine variants the GPU suites run on, as the environment a handle is compiled under (the variables are read
when a handle is compiled).  test_gpu_parity.py's `engine` fixture documents what each variant drives."""
import os

import pytest

VARIANTS = ["v2", "v1", "v2p", "u", "ur", "u23", "uh", "k", "p", "f", "auto"]

_ENGINE = {"v1": "v1", "u": "unit", "ur": "unit", "u23": "unit", "uh": "unit", "f": "filter", "k": "skip", "p": "pair"}


def use_variant(variant, monkeypatch):
    """Set (or clear) the variables of one variant; skips the test when AHA_TEST_ENGINES does not name it."""
    only = os.environ.get("AHA_TEST_ENGINES")  # (development: run the suite on some variants only, e.g. AHA_TEST_ENGINES=f,auto)
    if only and variant not in only.split(","):
        pytest.skip("variant not selected by AHA_TEST_ENGINES")
    if variant == "auto":
        monkeypatch.delenv("AHA_ENGINE", raising=False)
    else:
        monkeypatch.setenv("AHA_ENGINE", _ENGINE.get(variant, "v2"))
    if variant in ("u", "uh"):
        monkeypatch.setenv("AHA_UNIT_HEADER_BESIDE", "1" if variant == "uh" else "0")
    else:
        monkeypatch.delenv("AHA_UNIT_HEADER_BESIDE", raising=False)
    if variant == "u23":
        monkeypatch.setenv("AHA_UNIT_BASE_BITS", "23")
    else:
        monkeypatch.delenv("AHA_UNIT_BASE_BITS", raising=False)
    if variant == "ur":
        monkeypatch.setenv("AHA_UNIT_POST", "regroup")
    else:
        monkeypatch.delenv("AHA_UNIT_POST", raising=False)
    if variant == "v2p":
        monkeypatch.setenv("AHA_LDS_SLOTS", "1024")
    else:
        monkeypatch.delenv("AHA_LDS_SLOTS", raising=False)
    return variant
