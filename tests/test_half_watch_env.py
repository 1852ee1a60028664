"""CPU: the host side of audit.HalfRangeWatch that needs no device -- the HAMT_HALF_WATCH=1 switch (a fresh interpreter: it is read when
the module is imported), the package exports, enable / disable bookkeeping."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, **env):
    e = dict(os.environ)
    e.pop("HAMT_HALF_WATCH", None)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)


def test_env_switch_installs_one_enabled_watch_at_import():
    r = _run("from vln_hamt_amd import audit, blocks\n"
             "assert audit.ENV_WATCH is not None and audit.ACTIVE is audit.ENV_WATCH and audit.ENV_WATCH.enabled\n"
             "assert audit.ENV_WATCH.table is None and audit.ENV_WATCH.report() == []      # no device work at import\n"
             "print('ok')", HAMT_HALF_WATCH="1")
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])     # (and nothing is printed at exit: no layer ran)


def test_without_the_switch_no_watch_is_active():
    r = _run("from vln_hamt_amd import audit, blocks\nassert audit.ENV_WATCH is None and audit.ACTIVE is None\nprint('ok')")
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])


def test_package_exports_and_bookkeeping():
    import vln_hamt_amd
    from vln_hamt_amd import HalfRangeWarning, HalfRangeWatch, audit
    from vln_hamt_amd._lib import HamtError
    assert HalfRangeWatch is audit.HalfRangeWatch and issubclass(HalfRangeWarning, Warning)
    assert set(vln_hamt_amd.__all__) == {"HalfRangeWatch", "HalfRangeWarning"}
    with pytest.raises(AttributeError):
        vln_hamt_amd.no_such_name
    before = audit.ACTIVE
    a, b = HalfRangeWatch(), HalfRangeWatch()
    if before is None:
        with a:
            assert audit.ACTIVE is a and a.enabled and not b.enabled
            with pytest.raises(HamtError):
                b.enable()
        assert audit.ACTIVE is None and not a.enabled
    assert a.report() == [] and a.check() == [] and a.reset() is a
    with pytest.raises(HamtError):
        HalfRangeWatch(capacity=0)
    with pytest.raises(HamtError):
        a.promote(["no.such.layer"])
