"""The launches and checks of test_gpu_wgrad.py, importable (the test) and runnable (its one child for the one-phase 256 x 256 tile):

    HAMT_WGRAD_P8=0 python tests/_wgrad_gpu.py ratios.txt      # the 256-class cases of tests/_wgrad_ref.py on wgrad_grouped_kernel<256, 256, 2, 4>

hamt_wgrad_grouped(_ex) is called directly on buffers the caller owns.  Every operand is a column slice (8 columns in) of a wider
buffer that holds bf16 NaN everywhere else; dW has ldw > N and two rows below M, db and ss three floats behind them, the launch table
64 bytes behind it, and each of these is prefilled with a NaN bit pattern of its own and read back whole."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import torch

import _wgrad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN_DW, NAN_DB, NAN_SS, NAN_WIRE, NAN_OPERAND, TABLE_BYTE = 0x7FC5A5A5, 0x7FC3C3C3, 0x7FC99999, 0x7FD5, 0x7FC0, 0xA5
EXTRA_ROWS, GUARD, TABLE_GUARD = 2, 3, 64
QUANTITIES = ("dw", "db", "wire", "ss")
TWO_PHASE_256 = os.environ.get("HAMT_WGRAD_P8", "1") != "0"      # which 256-row kernel this process runs (the switch is read once per process)


def _L():
    from vln_hamt_amd import _lib as L
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def tile_setting(setting):
    """the setting's environment (read per call by the launcher), and nothing else of the launcher's switches"""
    saved = {k: os.environ.pop(k, None) for k in R.ENV_NAMES}
    os.environ.update(R.SETTINGS[setting][0])
    try:
        yield
    finally:
        for k in R.ENV_NAMES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Call:
    """the device buffers, their host prefill and the descriptors of one call's problems"""

    def __init__(self, probs, table_entries=None):
        L = _L()
        self.probs = list(probs)
        self.bufs, self.pre = [], []
        self.descs = (L.WgradDesc * max(1, len(self.probs)))()
        for i, p in enumerate(self.probs):
            off, ldy, ldx, ldy2, ldx2, ldw = R.leading_dims(p)
            b = {"dy": torch.empty(p.K * ldy, dtype=torch.int16, device=DEV), "x": torch.empty(p.K * ldx, dtype=torch.int16, device=DEV),
                 "dw": torch.empty((p.M + EXTRA_ROWS) * ldw, dtype=torch.int16 if p.wire else torch.int32, device=DEV),
                 "db": torch.empty(p.M + GUARD, dtype=torch.int32, device=DEV),
                 "ss": torch.empty(-(-p.M // 64) * -(-p.N // 128) + GUARD, dtype=torch.int32, device=DEV)}
            if p.K2:
                b["dy2"] = torch.empty(p.K2 * ldy2, dtype=torch.int16, device=DEV)
                b["x2"] = torch.empty(p.K2 * ldx2, dtype=torch.int16, device=DEV)
            assert all(t.data_ptr() % 16 == 0 for t in b.values())
            self.bufs.append(b)
            d = self.descs[i]
            d.dy, d.x, d.dw = b["dy"].data_ptr() + 2 * off, b["x"].data_ptr() + 2 * off, b["dw"].data_ptr()
            d.db, d.ss = (b["db"].data_ptr() if p.db else None), (b["ss"].data_ptr() if p.ss else None)
            d.M, d.N, d.K, d.ldy, d.ldx, d.ldw, d.accum_dw, d.accum_db = p.M, p.N, p.K, ldy, ldx, ldw, p.acc, int(p.db == 2)
            d.K_valid, d.wire_scale = p.kv, p.wire
            if p.K2:
                d.dy2, d.x2, d.K2, d.ldy2, d.ldx2, d.K2_valid = b["dy2"].data_ptr() + 2 * off, b["x2"].data_ptr() + 2 * off, p.K2, ldy2, ldx2, p.kv2
        n = sum(-(-p.M // 64) for p in self.probs) if table_entries is None else table_entries      # the contract's size: one entry per 64 output rows
        self.table_bytes = n * L.WGRAD_TABLE_ENTRY
        self.table = torch.full((self.table_bytes + TABLE_GUARD,), TABLE_BYTE, dtype=torch.uint8, device=DEV)
        assert self.table.data_ptr() % 16 == 0
        self.fill(self.probs)

    def fill(self, probs):
        """(re)write operands and prefill of every buffer IN PLACE from problems of the same shapes (other seeds: other contents)"""
        self.pre = []
        for p, q, b in zip(probs, self.probs, self.bufs):
            assert p._replace(seed=0) == q._replace(seed=0)
            off, ldy, ldx, ldy2, ldx2, ldw = R.leading_dims(p)
            dy, x, dy2, x2 = R.padded(p)
            _, _, _, _, dw0, db0 = R.operands(p.M, p.N, p.K, p.K2, p.seed)
            for name, bits, ld in (("dy", dy, ldy), ("x", x, ldx), ("dy2", dy2, ldy2), ("x2", x2, ldx2)):
                if bits is not None:
                    h = np.full((bits.shape[0], ld), NAN_OPERAND, dtype=np.uint16)
                    h[:, off:off + bits.shape[1]] = bits
                    b[name].copy_(_dev(h.view(np.int16).reshape(-1)))
            pre = {}
            if p.wire:
                pre["dw"] = np.full((p.M + EXTRA_ROWS, ldw), NAN_WIRE, dtype=np.uint16)
            else:
                pre["dw"] = np.full((p.M + EXTRA_ROWS, ldw), NAN_DW, dtype=np.uint32)
                if p.acc:
                    pre["dw"][:p.M, :p.N] = dw0.view(np.uint32)
            pre["db"] = np.full(p.M + GUARD, NAN_DB, dtype=np.uint32)
            if p.db == 2:
                pre["db"][:p.M] = db0.view(np.uint32)
            pre["ss"] = np.full(b["ss"].numel(), NAN_SS, dtype=np.uint32)
            pre["ss"][:-GUARD] = 0
            self.pre.append(pre)
        self.probs = list(probs)
        self.reset()

    def reset(self):
        for pre, b in zip(self.pre, self.bufs):
            b["dw"].copy_(_dev(pre["dw"].view(np.int16 if pre["dw"].dtype == np.uint16 else np.int32).reshape(-1)))
            b["db"].copy_(_dev(pre["db"].view(np.int32)))
            b["ss"].copy_(_dev(pre["ss"].view(np.int32)))

    def launch(self, phase=3, descs=None, n=None, table=0, table_bytes=None):
        """one hamt_wgrad_grouped(_ex) call; returns the tile rows of its kernel launches (hamt_debug_wgrad_times) and asserts their kernel
        family (hamt_debug_wgrad_variants).  Raises HamtError on a refusal."""
        L = _L()
        lib = L.load()
        descs = self.descs if descs is None else descs
        n = len(self.probs) if n is None else n
        tab = None if table is None else self.table.data_ptr() + table
        tb = self.table_bytes if table_bytes is None else table_bytes
        L.check(lib.hamt_debug_fill_lds(0x7FC07FC0, _stream()), "hamt_debug_fill_lds")      # every CU's LDS = bf16 NaN: a tile read before its DMA landed shows
        lib.hamt_debug_wgrad_timing(1)
        try:
            if phase == 3:
                L.check(lib.hamt_wgrad_grouped(n, descs, tab, tb, _stream()), "hamt_wgrad_grouped")
            else:
                L.check(lib.hamt_wgrad_grouped_ex(n, descs, tab, tb, phase, _stream()), "hamt_wgrad_grouped_ex")
            torch.cuda.synchronize()
            rows = (C.c_int * 8)()
            k = lib.hamt_debug_wgrad_times(None, rows, None, 8)
            assert 0 <= k <= 8, k
            two = (C.c_int * 8)()
            assert lib.hamt_debug_wgrad_variants(two, 8) == k
            # the kernel family of every launch: the two-phase kernel exists for 256 rows only, and 256 rows run on it unless HAMT_WGRAD_P8=0
            assert all(two[i] == int(rows[i] == 256 and TWO_PHASE_256) for i in range(k)), ([rows[i] for i in range(k)], [two[i] for i in range(k)])
            return sorted(rows[i] for i in range(k))
        finally:
            lib.hamt_debug_wgrad_timing(0)

    def read(self):
        """[{"dw", "db", "ss"}] bits of every buffer, whole"""
        torch.cuda.synchronize()
        out = []
        for p, pre, b in zip(self.probs, self.pre, self.bufs):
            dw = b["dw"].cpu().numpy()
            out.append({"dw": dw.view(np.uint16 if p.wire else np.uint32).reshape(pre["dw"].shape), "db": b["db"].cpu().numpy().view(np.uint32),
                        "ss": b["ss"].cpu().numpy().view(np.uint32)})
        return out

    def table_guard_intact(self):
        return bool((self.table[self.table_bytes:] == TABLE_BYTE).all())

    def untouched(self, got=None):
        """names of the buffers that differ from their prefill anywhere"""
        got = self.read() if got is None else got
        return [(i, k) for i, (g, pre) in enumerate(zip(got, self.pre)) for k in ("dw", "db", "ss") if not np.array_equal(g[k], pre[k])]


def new_worst():
    """{quantity: worst error / bound so far}; -1: no output of that kind checked"""
    return dict.fromkeys(QUANTITIES, -1.0)


def ratios(worst):
    return ", ".join(f"{q} {worst[q]:.4f}" if worst[q] >= 0 else f"{q} -" for q in QUANTITIES)


def same_bits(a, b):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("dw", "db", "ss")) and len(a) == len(b)


def check_problem(tag, p, pre, got, worst):
    """one problem's outputs against tests/_wgrad_ref.py; the worst error / bound per quantity goes into `worst`"""
    M, N, bm = p.M, p.N, p.rows
    bn = R.bn_of(bm)
    W = R.want_and_bounds(p)
    inside = np.zeros(pre["dw"].shape, dtype=bool)
    inside[:M, :N] = True
    assert np.array_equal(got["dw"][~inside], pre["dw"][~inside]), f"{tag}: dW was written outside [M, N) (ldw {pre['dw'].shape[1]})"
    if p.wire:
        wire = R.bf16_value(got["dw"][:M, :N]).astype(np.float64)
        assert np.isfinite(wire).all(), f"{tag}: {np.count_nonzero(~np.isfinite(wire))} wire elements unwritten or not finite"
        worst["wire"] = max(worst["wire"], float(np.max(np.abs(wire - W["wire"]) / W["wire_bound"])))
    else:
        dw = np.ascontiguousarray(got["dw"][:M, :N]).view(np.float32)
        assert np.isfinite(dw).all(), f"{tag}: {np.count_nonzero(~np.isfinite(dw))} elements of dW unwritten or not finite"
        worst["dw"] = max(worst["dw"], float(np.max(np.abs(dw.astype(np.float64) - W["dw"]) / W["dw_bound"])))
    if p.db:
        assert np.array_equal(got["db"][M:], pre["db"][M:]), f"{tag}: db was written behind row M"
        db = got["db"][:M].view(np.float32)
        assert np.isfinite(db).all(), f"{tag}: rows {np.flatnonzero(~np.isfinite(db))[:8]} of db unwritten or not finite"
        worst["db"] = max(worst["db"], float(np.max(np.abs(db.astype(np.float64) - W["db"]) / W["db_bound"])))
    else:
        assert np.array_equal(got["db"], pre["db"]), f"{tag}: db was written without a db pointer"
    if p.ss:
        assert np.array_equal(got["ss"][-GUARD:], pre["ss"][-GUARD:]), f"{tag}: ss was written behind its last slot"
        lay = R.ss_layout(M, N, bm, bn)
        ss = got["ss"][:-GUARD].reshape(lay.shape)
        assert (ss[~lay] == 0).all(), f"{tag}: ss slots that no {bm} x {bn} tile owns are not +0.0: {np.argwhere((ss != 0) & ~lay)[:6].tolist()}"
        ssf = ss.view(np.float32)
        assert np.isfinite(ssf).all() and (ssf[lay] > 0).all(), f"{tag}: origin slots of the {bm} x {bn} tiles empty: {np.argwhere((ssf == 0) & lay)[:6].tolist()}"
        want = R.ss_f64(dw, bm, bn)              # of the fp32 dW the kernel itself stored
        worst["ss"] = max(worst["ss"], float(np.max(np.abs(ssf[lay].astype(np.float64) - want[lay]) / R.ss_bound(want[lay], bm))))
    else:
        assert np.array_equal(got["ss"], pre["ss"]), f"{tag}: ss was written without an ss pointer (or next to a wire output)"


def run_case(setting, cid, probs, twice=True):
    """one call under a tile setting, every check; returns ({quantity: worst error / bound}, the outputs' bits)"""
    with tile_setting(setting):
        call = Call(probs)
        rows = call.launch()
        got = call.read()
        assert rows == sorted({p.rows for p in probs}), f"{setting} {cid}: kernel launches on tile rows {rows}, the case names {sorted({p.rows for p in probs})}"
        assert call.table_guard_intact(), f"{setting} {cid}: the table was written behind its size"
        worst = new_worst()
        for i, (p, pre, g) in enumerate(zip(probs, call.pre, got)):
            check_problem(f"{setting} {cid} [{i}] {p}", p, pre, g, worst)
        if twice:                                # the same call again, from the same prefill: the same bits
            call.reset()
            assert call.launch() == rows
            assert same_bits(call.read(), got), f"{setting} {cid}: a second call gave other bits"
    print(f"[wgrad {setting} {cid}] {len(probs)} problems, tile rows {rows}, worst error / bound: {ratios(worst)}")
    assert all(worst[q] <= 1.0 for q in QUANTITIES), (setting, cid, worst)
    return worst, got


if __name__ == "__main__":      # child of test_gpu_wgrad.py: the one-phase 256 x 256 tile (HAMT_WGRAD_P8=0, read once per process)
    sys.path.insert(0, ROOT)
    assert os.environ.get("HAMT_WGRAD_P8") == "0" and not TWO_PHASE_256
    with open(sys.argv[1], "w") as f:
        for cid, probs in R.cases("256"):
            if any(p.rows == 256 for p in probs):
                worst, _ = run_case("256", cid, probs)
                f.write(f"256 {cid}: {ratios(worst)}\n")
                f.flush()
