"""Shared by tests/test_ralamb_items.py (CPU) and tests/test_gpu_ralamb_items.py: the small arena the item-range kernels of
optim/rangerlars.py are tested on, two steps' worth of tables for it, and a numpy float64 restatement of the owned-item update
("moments per item range, sum the partial slots, trust ratios, apply per item range"); the whole-arena one it is compared with
is tests/test_gpu_rangerlars.py's `_restate`."""
import numpy as np

# element counts: two tiny tensors, exactly one item, a full item plus a 2-float4 item, three items, an INACTIVE tensor, one with active == 2
SIZES = [8, 24, 4096, 4104, 12288, 40, 8200]
INACTIVE, KEPT = 5, 6
N = 29184                                              # 57 * 512: the tail is alignment padding of the last tensor
ENDS = np.array([8, 32, 4128, 8232, 20520, 20560, N])
BEGINS = np.array([0, 8, 32, 4128, 8232, 20520, 20560])
# one cut inside the 24-element tensor, one on a tensor boundary, one in the middle of the first item of the 12288-element tensor
CUTS = (16, 4128, 8232 + 2048)
SEGMENTS = [(0, 16), (16, 4128 - 16), (4128, 8232 + 2048 - 4128), (8232 + 2048, N - 8232 - 2048)]     # the cut intervals as (first, count)
MIDDLE = 2                                             # the segment "one range touches nothing else" runs alone
B1, B2, EPS, MAX_NORM, GSQ = 0.9, 0.98, 1e-8, 1.0, 25.0        # clip coefficient 1 / (5 + 1e-6) < 1: the clip is active

# recorded from item_table(ends, n) as it was before it took `cuts` (the parent commit's function), for the arenas named beside them
RECORDED = {
    # tests/test_rangerlars.py::test_item_table_layout's arena
    (8, 8, 4096, 4104, 16400, 53280): (17, [0, 2, 1024, 1026, 2050, 3074, 4098, 4100, 5124, 6148, 7172, 8196, 9220, 10244, 11268, 12292, 13316,
                                            13320, 0, 2, 3, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 0, 1, 1, 2, 3, 7, 17]),
    # ENDS above
    (8, 32, 4128, 8232, 20520, 20560, 29184): (12, [0, 2, 8, 1032, 2056, 2058, 3082, 4106, 5130, 5140, 6164, 7188, 7296, 0, 1, 2, 3, 3, 4, 4,
                                                    4, 5, 6, 6, 6, 0, 1, 2, 3, 5, 8, 9, 12]),
    # TWO_REGION_ENDS below
    (12288, 20480, 21504, 21512, 21536, 22536, 27648): (11, [0, 1024, 2048, 3072, 4096, 5120, 5376, 5378, 5384, 5634, 6658, 6912, 0, 0, 0, 1,
                                                             1, 2, 3, 4, 5, 6, 6, 0, 3, 5, 6, 7, 8, 9, 11]),
}
# an arena with both regions: GEMM weights [0, 21504), fp32-read tensors behind them; both ends multiples of 512
TWO_REGION_ENDS, TWO_REGION_NA, TWO_REGION_N = np.array([12288, 20480, 21504, 21512, 21536, 22536, 27648]), 21504, 27648


def make_case(step: int):
    """arenas and tables of "step" 0 / 1: between them every active tensor changes its N_sma branch and its Lookahead action, so that
    the two cover rect off / on x none / create / interpolate, with and without weight decay"""
    rng = np.random.Generator(np.random.PCG64(23))
    nt = len(SIZES)
    active = np.ones(nt, dtype=np.float32)
    active[INACTIVE], active[KEPT] = 0, 2
    rect = np.array([(i + step) % 2 for i in range(nt)], dtype=np.float32)
    action = np.array([(i + 2 * step) % 3 for i in range(nt)], dtype=np.float32)
    lr = np.where(np.arange(nt) % 3 == 0, 3e-3, 1e-3)
    s = np.where(rect == 1, 0.37, 1.9)
    wd = np.where(np.arange(nt) % 2 == 1, 0.0, 0.01)
    alpha = np.where(np.arange(nt) % 2 == 0, 0.5, 0.25)
    hyp = np.stack([lr, s * lr, wd, active], 1).astype(np.float32)
    rl = np.stack([rect, action, alpha, -wd * lr], 1).astype(np.float32)
    p, g, m, v, slow = (np.zeros(N, np.float32) for _ in range(5))
    for i, sz in enumerate(SIZES):
        lo, hi = BEGINS[i], ENDS[i]
        if active[i] == 0:
            for a in (p, g, m, v, slow):
                a[lo:hi] = np.nan
            continue
        p[lo:lo + sz] = rng.normal(0, 0.02, sz)
        g[lo:lo + sz] = rng.normal(0, 1e-2, sz)
        m[lo:lo + sz] = rng.normal(0, 1e-3, sz)
        v[lo:lo + sz] = rng.uniform(1e-7, 1e-4, sz)
        slow[lo:lo + sz] = p[lo:lo + sz] + rng.normal(0, 1e-3, sz)
    return dict(n=N, ends=ENDS, begins=list(BEGINS), active=active, rect=rect, action=action, hyp=hyp, rl=rl, p=p, g=g, m=m, v=v, slow=slow)


def split(tab, nitems, nparams):
    return tab[:nitems + 1].astype(np.int64), tab[nitems + 1:2 * nitems + 1], tab[2 * nitems + 1:2 * nitems + nparams + 2]


class ItemRestatement:
    """float64 state of one update, advanced pass by pass over item ranges the way the three entry points advance the arenas"""

    def __init__(self, c, tab, nitems, stats0=None):
        self.c, self.nitems = c, nitems
        self.starts, self.param, self.first = split(tab, nitems, len(c["ends"]))
        self.a = {k: c[k].astype(np.float64).copy() for k in ("p", "g", "m", "v", "slow")}
        self.partials = np.full((nitems, 2), np.nan)
        self.stats = np.full((len(c["ends"]), 3), 7.0) if stats0 is None else stats0.copy()
        self.coef = min(1.0, MAX_NORM / (float(np.sqrt(np.float32(GSQ))) + 1e-6))

    def _row(self, q):
        lr, slr, wd = (float(x) for x in self.c["hyp"][q, :3])
        return lr, slr, wd

    def moments(self, item_first, item_count):
        a, c = self.a, self.c
        for j in range(item_first, item_first + item_count):
            q = int(self.param[j])
            if c["active"][q] == 0:
                continue
            sl = slice(4 * self.starts[j], 4 * self.starts[j + 1])
            lr, slr, wd = self._row(q)
            gg = a["g"][sl] * self.coef
            a["m"][sl] = B1 * a["m"][sl] + (1 - B1) * gg
            a["v"][sl] = B2 * a["v"][sl] + (1 - B2) * gg * gg
            pd = a["p"][sl] - wd * lr * a["p"][sl]
            u = a["m"][sl] / (np.sqrt(a["v"][sl]) + EPS) if c["rect"][q] else a["m"][sl]
            self.partials[j] = (pd * pd).sum(), ((pd - slr * u) ** 2).sum()
            if c["active"][q] == 1:
                a["g"][sl] = 0.0

    def trust(self):
        for q in range(len(self.c["ends"])):
            if self.c["active"][q] == 0:
                continue
            t = self.partials[self.first[q]:self.first[q + 1]].sum(0)
            wn, an = min(np.sqrt(t[0]), 10.0), np.sqrt(t[1])
            self.stats[q] = wn, an, (1.0 if wn == 0 or an == 0 else wn / an)

    def apply(self, item_first, item_count):
        a, c = self.a, self.c
        for j in range(item_first, item_first + item_count):
            q = int(self.param[j])
            if c["active"][q] == 0:
                continue
            sl = slice(4 * self.starts[j], 4 * self.starts[j + 1])
            lr, slr, wd = self._row(q)
            pd = a["p"][sl] - wd * lr * a["p"][sl]
            u = a["m"][sl] / (np.sqrt(a["v"][sl]) + EPS) if c["rect"][q] else a["m"][sl]
            pn = pd - slr * self.stats[q, 2] * u
            act = int(c["action"][q])
            if act == 1:
                a["slow"][sl] = pn
            elif act == 2:
                pn = a["slow"][sl] + float(c["rl"][q, 2]) * (pn - a["slow"][sl])
                a["slow"][sl] = pn
            a["p"][sl] = pn

