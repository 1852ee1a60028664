"""Range watch on the half-precision dense outputs of the bf16 path.

The three dense layers that feed a LayerNorm (the attention output projection of blocks.SelfAttnBlockFn / CrossAttnBlockFn, the second
FFN layer of blocks.FfnBlockFn) write IEEE half (blocks.O_DTYPE), and the store clamps at +-65504.  With random weights those outputs
are O(1 .. 100); a trained checkpoint with outlier channels may reach the limit, and a clamped value is a wrong LayerNorm row that
nothing reports.  `HalfRangeWatch` makes it visible and fixes it per layer:

    watch = HalfRangeWatch(model)
    with watch:                          # or watch.enable() / watch.disable()
        loss = model(batch, task, True).mean(); loss.backward()
    for name, at_limit, nonfinite, max_abs, calls in watch.report():   # ONE device-to-host copy
        ...
    watch.check()                        # HalfRangeWarning once per offending layer; returns their names
    watch.promote_flagged()              # those layers allocate fp32 outputs from now on (+ 2 bytes per element written and read)

While a watch is enabled each of the three sites launches hamt_range_audit (csrc/audit.hip) on its output right behind the GEMM: one
small kernel on the current stream that adds into that layer's row of a device table -- elements at the limit (|x| == 65504: what the
clamp turns every overflow into; a value that merely rounds to 65504 is counted too, so the count is an upper bound), non-finite
elements, the largest finite magnitude, calls.  Nothing is read back before `report()`.  With no watch enabled the sites cost one
`is None` test and launch exactly what they launched before.

A site is one dense layer, identified by its weight Parameter; the two sides of a cross-modal layer share weights and so a row.

Graph capture: the audit is an ordinary launch, so a graph captured while a watch is enabled audits on EVERY replay (into that watch's
table, enabled or not by then), and a graph captured while no watch is enabled never audits.  Rows are handed out on the host, which
works during a capture; the table itself must exist before one (it does after `enable()` on a machine with a GPU).  Promotion changes
what a pass allocates: it takes effect with the next eager pass or the next capture -- graphs captured before must be captured again.

HAMT_HALF_WATCH=1 installs one process-wide enabled watch when this module is imported and calls its `check()` at exit: an unmodified
training script pointed at a checkpoint then says which layers, if any, need promotion.  blocks.O_DTYPE and its two environment
switches (HAMT_DENSE_OUT_F32 / HAMT_DENSE_OUT_BF16) stay the default every layer without a promotion takes.
"""
from __future__ import annotations

import atexit
import os
import warnings
import weakref
from collections import namedtuple

import torch

from . import _lib as L
from . import ops

HALF_MAX = 65504.0
PROMOTED_ATTR = "_hamt_o_f32"       # set on a dense layer's weight Parameter by promote(); read by blocks._o_dtype

ACTIVE = None                       # the enabled watch; blocks.py tests `audit.ACTIVE is not None` at each site

SiteRange = namedtuple("SiteRange", "name at_limit nonfinite max_abs calls")

_MODELS = weakref.WeakSet()         # every modeling.HamtPreTrainedModel alive: how the HAMT_HALF_WATCH watch, built before any model, names its rows


def note_model(model):
    _MODELS.add(model)


class HalfRangeWarning(UserWarning):
    """a dense output reached half's limit (or holds non-finite values): its LayerNorm rows are wrong until the layer is promoted"""


class HalfRangeWatch:
    """See the module docstring.  `model`: names the rows by `named_parameters()` (without it: "site0", "site1", ... in the order the
    layers first ran).  `capacity`: rows of the device table, int64 [capacity, 4]; a layer seen beyond it raises HamtError."""

    def __init__(self, model=None, capacity=512, _process_wide=False):
        self.model = model
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise L.HamtError(f"HalfRangeWatch: capacity must be at least 1, got {capacity}")
        self.table = None
        self._rows = []             # per site: its row of the table (a view, made once)
        self._index = {}            # id(weight Parameter) -> site
        self._params = []           # the Parameters themselves: keeps the ids above theirs
        self._warned = set()
        self._process_wide = _process_wide      # the HAMT_HALF_WATCH watch: no device work before a layer runs, rows named through _MODELS

    # ------------------------------------------------------------------ switching
    def _device(self):
        if self.model is not None:
            for p in self.model.parameters():
                if p.is_cuda:
                    return p.device
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None

    def _make_table(self, dev):
        if torch.cuda.is_current_stream_capturing():
            raise L.HamtError("HalfRangeWatch: the record table must exist before a graph capture (memory allocated inside one belongs to "
                              "the graph's pool): call enable() or run one eager pass first")
        self.table = torch.zeros(self.capacity, ops.RANGE_REC, dtype=torch.int64, device=dev)

    def enable(self):
        global ACTIVE
        if ACTIVE is not None and ACTIVE is not self:
            raise L.HamtError("HalfRangeWatch.enable: another watch is enabled (disable it first; one watch at a time)")
        if self.table is None and not self._process_wide:
            dev = self._device()
            if dev is not None:
                self._make_table(dev)
        ACTIVE = self
        return self

    def disable(self):
        global ACTIVE
        if ACTIVE is self:
            ACTIVE = None
        return self

    @property
    def enabled(self):
        return ACTIVE is self

    def __enter__(self):
        return self.enable()

    def __exit__(self, *exc):
        self.disable()
        return False

    # ------------------------------------------------------------------ the sites' side
    def row(self, w):
        """the record of the dense layer with weight `w` (int64 [4] on the device); a layer seen for the first time takes the next row --
        host bookkeeping only"""
        i = self._index.get(id(w))
        if i is None:
            i = len(self._rows)
            if i >= self.capacity:
                raise L.HamtError(f"HalfRangeWatch: more than capacity={self.capacity} dense layers; build the watch with a larger capacity")
            if self.table is None:
                self._make_table(w.device)
            if w.device != self.table.device:
                raise L.HamtError(f"HalfRangeWatch: the table is on {self.table.device}, this layer on {w.device} (one watch per device)")
            self._index[id(w)] = i
            self._params.append(w)
            self._rows.append(self.table[i])
        return self._rows[i]

    # ------------------------------------------------------------------ reading
    def _models(self):
        return [self.model] if self.model is not None else (list(_MODELS) if self._process_wide else [])

    def _names(self):
        """the model's parameter names, or "site<i>" in first-seen order without a model; the process-wide watch, which is built before any
        model, takes the names the models alive in the process give (the longest wins: the outermost model's, with its prefixes)"""
        by_id = {}
        for m in self._models():
            for n, p in m.named_parameters():
                if len(n) > len(by_id.get(id(p), "")):
                    by_id[id(p)] = n
        return [by_id.get(id(p), f"site{i}") for i, p in enumerate(self._params)]

    def report(self):
        """[SiteRange(name, at_limit, nonfinite, max_abs, calls)] for every layer seen, in first-seen order.  One device-to-host copy,
        which waits for the audits in front of it on the current stream."""
        n = len(self._rows)
        if n == 0:
            return []
        host = self.table[:n].cpu()
        max_abs = host[:, 2].to(torch.int32).view(torch.float32).tolist()
        cnt = host.tolist()
        return [SiteRange(name, cnt[i][0], cnt[i][1], float(max_abs[i]), cnt[i][3]) for i, name in enumerate(self._names())]

    def check(self):
        """names of the layers with elements at the limit or non-finite; a HalfRangeWarning for each, once per layer until reset()"""
        bad = []
        for r in self.report():
            if r.at_limit > 0 or r.nonfinite > 0:
                bad.append(r.name)
                if r.name not in self._warned:
                    self._warned.add(r.name)
                    warnings.warn(HalfRangeWarning(
                        f"{r.name}: {r.at_limit} output element(s) at half's limit +-{HALF_MAX:.0f} (clamped, or rounded to it), {r.nonfinite} "
                        f"non-finite, largest finite |x| {r.max_abs:.6g} over {r.calls} call(s) -- the LayerNorm behind this layer sees wrong "
                        f"values; HalfRangeWatch.promote(['{r.name}']) gives it fp32 outputs"), stacklevel=2)
        return bad

    def reset(self):
        """zero every record (on the current stream); the layers keep their rows and their promotions"""
        if self.table is not None:
            self.table.zero_()
        self._warned.clear()
        return self

    # ------------------------------------------------------------------ promotion
    def promote(self, names, on=True):
        """The named layers (names as report() gives them, or the weight Parameters themselves) allocate their output as fp32 from the
        next eager pass or the next capture on: + 2 bytes per element written by the GEMM and read by the LayerNorm, and the saved
        pre-LN sum of that layer fp32 too.  Already-captured graphs keep what they captured: capture them again.  `on=False` takes a
        promotion back.  The mark sits on the Parameter, so it outlives this watch."""
        if isinstance(names, (str, torch.Tensor)):
            names = [names]
        by_name = dict(zip(self._names(), self._params))
        for m in self._models():
            for n, p in m.named_parameters():
                by_name.setdefault(n, p)
        done = []
        for n in names:
            p = n if torch.is_tensor(n) else by_name.get(n)
            if p is None:
                raise L.HamtError(f"HalfRangeWatch.promote: no dense layer named {n!r} (known: report()'s names"
                                  + (", the model's parameter names)" if self.model is not None else ")"))
            if on:
                setattr(p, PROMOTED_ATTR, True)
            elif hasattr(p, PROMOTED_ATTR):
                delattr(p, PROMOTED_ATTR)
            done.append(n)
        return done

    def promote_flagged(self):
        return self.promote(self.check())


# ---------------------------------------------------------------------------------------- HAMT_HALF_WATCH=1
ENV_WATCH = None


def _check_at_exit():
    w = ENV_WATCH
    if w is None or not w._rows:
        return
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("always", HalfRangeWarning)
            bad = w.check()
        rows = w.report()
        print(f"[HAMT_HALF_WATCH] {len(rows)} dense layer(s) watched, {len(bad)} at half's limit or non-finite; largest |x| "
              f"{max(r.max_abs for r in rows):.6g}", flush=True)
    except Exception as e:      # (the device may be gone at exit: say so, never turn a finished run into a failed one)
        print(f"[HAMT_HALF_WATCH] could not read the records at exit: {e}", flush=True)


if os.environ.get("HAMT_HALF_WATCH") == "1":
    ENV_WATCH = HalfRangeWatch(_process_wide=True).enable()      # (no device work at import: the table is made when the first layer runs)
    atexit.register(_check_at_exit)
