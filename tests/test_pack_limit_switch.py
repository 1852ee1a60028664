"""Not gpu: HAMT_PACK_MAX_LEN is read when model/vilmodel.py is imported -- 128 without it, 128 or 256 with it, anything else refused.
One fresh interpreter per value (the module is imported once per process)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = "from vln_hamt_amd.model import vilmodel; print('limit', vilmodel.PACK_MAX_LEN)"


def _import_with(value):
    env = {k: v for k, v in os.environ.items() if k != "HAMT_PACK_MAX_LEN"}
    if value is not None:
        env["HAMT_PACK_MAX_LEN"] = value
    return subprocess.run([sys.executable, "-c", CODE], cwd=ROOT, env=env, capture_output=True, text=True)


@pytest.mark.parametrize("value,limit", [(None, 128), ("128", 128), ("256", 256)])
def test_the_limit_follows_the_variable(value, limit):
    r = _import_with(value)
    assert r.returncode == 0 and f"limit {limit}" in r.stdout, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("value", ["200", "512", "long"])
def test_other_values_are_refused_at_import(value):
    r = _import_with(value)
    assert r.returncode != 0 and "HAMT_PACK_MAX_LEN" in r.stderr and "ValueError" in r.stderr, (r.stdout, r.stderr[-2000:])
