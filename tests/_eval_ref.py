"""float64 restatements of the three validation accumulations (csrc/eval.hip, ops.eval_ce / eval_kl / eval_mse_cols) on top of
_smallops_ref.ce_f64 / kl_f64 / mse32, the arg-max rule, the mistakes the cases have to catch, and the case builders shared by
test_eval_ref.py (CPU), test_gpu_eval.py and tools/gen_validate_golden.py.  Nothing here touches torch, the GPU or the package under test."""
import functools

import numpy as np

from _smallops_ref import CE_LOSS_BOUND, F32, KL_LOSS_BOUND, PAD_VALUE, ce_f64, kl_f64, lse_f64, mse32, row_unit

MLM_C = 30522


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---------------------------------------------------------------------------------------------- the arg-max rule
def argmax_rows(x, highest=False, drop_tail=False):
    """scores.max(dim=-1)[1]: the LOWEST index among a row's maxima; -1 for a row with a NaN (never correct).  The mistakes:
    highest = the highest index among them, drop_tail = the columns past 256 floor(C / 256) are never looked at (C >= 256)."""
    x = np.asarray(x, dtype=np.float64)
    R, C = x.shape
    if drop_tail and C >= 256:
        x = x[:, :256 * (C // 256)]
    if x.shape[1] == 0:
        return np.full(R, -1, dtype=np.int64)
    a = (x.shape[1] - 1 - np.argmax(x[:, ::-1], axis=1)) if highest else np.argmax(x, axis=1)
    return np.where(np.isnan(x).any(axis=1), -1, a).astype(np.int64)


def _rows_of(buf, C, ld, stride_is_C=False):
    """the [R, C] rows of a flat [R, ld] buffer; the mistake stride_is_C reads row r at r C"""
    buf = np.asarray(buf)
    R = buf.shape[0]
    if not stride_is_C:
        return buf[:, :C]
    flat = buf.reshape(-1)
    return np.stack([flat[r * C:r * C + C] for r in range(R)]) if R else buf[:, :C]


# ---------------------------------------------------------------------------------------------- the three accumulations
def eval_ce_f64(buf, C, label, highest=False, drop_tail=False, count_ignored=False, add_ignored=False, stride_is_C=False):
    """-> (loss sum, n_correct, n, bound): float64 sum of ce_f64's row losses over the rows with label >= 0, the rows among them whose
    arg-max is the label, their number, and sum_r CE_LOSS_BOUND row_unit_r over them.  A label >= C gives NaN."""
    x = _rows_of(buf, C, buf.shape[1], stride_is_C)
    label = np.asarray(label, dtype=np.int64)
    loss, lse, _ = ce_f64(x, label)
    loss = np.where(label >= C, np.nan, loss)
    live = label >= 0
    if add_ignored:                                               # the ordinary loss of an ignored row, against class 0
        loss = np.where(live, loss, ce_f64(x, np.zeros_like(label))[0])
    pick = np.ones_like(live) if add_ignored else live
    total = float(np.sum(loss[pick], dtype=np.float64))
    correct = int(((argmax_rows(x, highest, drop_tail) == label) & live).sum())
    n = int(len(label) if count_ignored else live.sum())
    bound = float((CE_LOSS_BOUND * row_unit(x, lse))[live].sum())
    return total, correct, n, bound


def eval_kl_f64(x, t, target_from_pred=False):
    """-> (loss sum, n_correct, n = R, bound).  The mistake target_from_pred takes the target's arg-max from the prediction."""
    x, t = np.asarray(x), np.asarray(t, dtype=F32)
    loss, lse, _ = kl_f64(x, t)
    ax = argmax_rows(x)
    at = ax if target_from_pred else argmax_rows(t)
    return float(loss.sum()), int(((ax == at) & (ax >= 0)).sum()), int(x.shape[0]), float((KL_LOSS_BOUND * row_unit(x, lse)).sum())


def eval_mse_cols_f64(x, t, swap=False):
    """per column: the float64 sum of the fp32 terms d * d (mse32).  The mistake swap exchanges the first two columns."""
    term = mse32(x, t).astype(np.float64)
    s = term.sum(axis=0)
    if swap and len(s) >= 2:
        s[[0, 1]] = s[[1, 0]]
    return s


# ---------------------------------------------------------------------------------------------- cases
ARGMAX_C = (1, 2, 63, 64, 65, 255, 256, 257, 513, MLM_C)


def _argmax_case(C, seed):
    """rows with the maximum at column 0, C - 1, 255, 256, and exact ties between c and c + 256 (one thread of the 256), 10 and 70 (two
    waves), 3 and 4 (neighbouring lanes), each labelled with its lower column (correct); the 10 / 70 tie once more with its higher one (not)"""
    rng = _rng(seed)
    peaks = [((0,), 0), ((C - 1,), C - 1)]
    for c in (255, 256):
        if c < C:
            peaks.append(((c,), c))
    for lo, hi in ((5, 261), (C - 257, C - 1), (10, 70), (3, 4)):
        if 0 <= lo < hi < C:
            peaks.append(((lo, hi), lo))
            if (lo, hi) == (10, 70):
                peaks.append(((lo, hi), hi))
    peaks.append(((), int(rng.integers(C))))                       # an ordinary row with a random label
    R, ld = len(peaks), C + 3
    buf = np.full((R, ld), PAD_VALUE, dtype=F32)
    label = np.zeros(R, dtype=np.int64)
    for r, (cols, lab) in enumerate(peaks):
        x = rng.standard_normal(C).astype(F32)
        for c in cols:
            x[c] = F32(x.max() + 2.0) if c == cols[0] else x[cols[0]]
        buf[r, :C] = x
        label[r] = lab
    return dict(name=f"argmax {R}x{C}", R=R, C=C, ld=ld, buf=buf, label=label, peaks=peaks)


@functools.lru_cache(maxsize=None)
def argmax_cases():
    return [_argmax_case(C, 100 + i) for i, C in enumerate(ARGMAX_C)]


FOLD_R = (0, 1, 255, 256, 257, 4097)


@functools.lru_cache(maxsize=None)
def fold_cases():
    """row counts around the fold's 256 threads at C = 5 (in rows of 8 floats); every seventh label ignored"""
    out = []
    for i, R in enumerate(FOLD_R):
        rng = _rng(200 + i)
        buf = np.full((R, 8), PAD_VALUE, dtype=F32)
        buf[:, :5] = (3 * rng.standard_normal((R, 5))).astype(F32)
        label = rng.integers(0, 5, size=R).astype(np.int64)
        label[3::7] = -100
        out.append(dict(name=f"fold {R}x5", R=R, C=5, ld=8, buf=buf, label=label))
    return out


def split_finite(c):
    """a _smallops_ref.ce_cases() case -> (rows whose loss is finite or ignored, rows that must give inf / NaN)"""
    loss = ce_f64(c["x"], c["label"])[0]
    fin = np.isfinite(loss)
    return np.flatnonzero(fin), np.flatnonzero(~fin)


@functools.lru_cache(maxsize=None)
def kl_argmax_case():
    """C = 1000 rows where the prediction's and the target's arg-max agree, disagree, and tie: a tied prediction (lowest index decides)
    against a target at the lower / the higher column; an all-zero target (arg-max 0) against a prediction peaking at 0 and elsewhere"""
    rng = _rng(300)
    R, C = 8, 1000
    x = (2 * rng.standard_normal((R, C))).astype(F32)
    z = 2 * rng.standard_normal((R, C))
    t = np.exp(z - z.max(axis=1, keepdims=True))
    t = (t / t.sum(axis=1, keepdims=True)).astype(F32)
    top = lambda a: F32(a.max() + 2.0)
    t[0, 17] = 0.5; x[0, 17] = top(x[0])                           # agree
    t[1, 17] = 0.5; x[1, 900] = top(x[1])                          # disagree
    x[2, 300] = top(x[2]); x[2, 556] = x[2, 300]; t[2, 300] = 0.5  # tied prediction, target on the lower column: agree
    x[3, 300] = top(x[3]); x[3, 556] = x[3, 300]; t[3, 556] = 0.5  # ... on the higher column: disagree
    t[4] = 0; x[4, 0] = top(x[4])                                  # all-zero target: its arg-max is column 0
    t[5] = 0; x[5, 999] = top(x[5])
    t[6] = 0; t[6, 999] = 1.0; x[6, 999] = top(x[6])               # one-hot target at the last column
    t[7, 4] = 0.25; t[7, 260] = 0.25; x[7, 260] = top(x[7])        # tied TARGET: lowest index 4, prediction at 260: disagree
    return dict(name="kl argmax 8x1000", R=R, C=C, x=x, t=t, t32=t)


MSE_COLS_C, MSE_COLS_R = (1, 2, 3, 4), (1, 255, 257, 2304)


def mse_cols_case(R, C, seed=400):
    """values around 1e-3 and around 1e3 in the first column, O(1) elsewhere, in buffers of row stride C + 1"""
    rng = _rng(seed + 10 * R + C)
    xb, tb = (np.full((R, C + 1), PAD_VALUE, dtype=F32) for _ in range(2))
    x = rng.standard_normal((R, C))
    t = rng.standard_normal((R, C))
    scale = np.where(np.arange(R) % 2 == 0, 1e-3, 1e3)
    x[:, 0] *= scale
    t[:, 0] *= scale
    xb[:, :C], tb[:, :C] = x.astype(F32), t.astype(F32)
    return dict(name=f"mse {R}x{C}", R=R, C=C, xb=xb, tb=tb, x=xb[:, :C], t=tb[:, :C])


# ---------------------------------------------------------------------------------------------- the golden's scripted MLM rows
def mlm_scripted_scores(seed, labels):
    """the 30 522-wide rows of one scripted MLM batch, regenerated from `seed` (they are not stored): 3 N(0, 1), and in every second row
    the label's logit lifted above the row's maximum, so that the label is the arg-max there and (almost surely) not in the others"""
    labels = np.asarray(labels, dtype=np.int64)
    x = (3 * _rng(seed).standard_normal((len(labels), MLM_C))).astype(F32)
    for r in range(0, len(labels), 2):
        x[r, labels[r]] = F32(x[r].max() + 1.5)
    return x


def top_two_gap_ok(x, ulps=64):
    """the generator's condition on its CE / KL rows: the two largest logits of every finite row are bit-equal or more than `ulps`
    fp32 ulps of max(1, |lse|, max |x|) apart, so that fp32 log_softmax cannot merge them and the reference's arg-max is the exact one"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0 or x.shape[1] < 2:
        return True
    lse = lse_f64(x)
    unit = row_unit(x, lse)
    top = np.sort(x, axis=1)[:, -2:]
    gap = top[:, 1] - top[:, 0]
    ok = (gap == 0) | (gap > ulps * unit) | ~np.isfinite(lse) | np.isnan(gap)
    return bool(ok.all())


# ---------------------------------------------------------------------------------------------- the golden (tests/golden/validate.npz)
GOLDEN_TAGS = {"mlm": "ce", "sap": "ce", "sapnan": "ce", "itm": "ce", "mrc": "kl", "sar": "mse", "sprel": "mse", "sprel3d": "mse"}
EPS32 = 2.0 ** -23


def golden_batches(store, tag):
    """the scripted batches of one task as numpy arrays: what the stand-in model returns (`scores`, and `labels` / `targets` for the
    2-tuples) and what the batch itself carries"""
    out = []
    for i in range(int(store[f"{tag}/n_batches"])):
        g = lambda k: store[f"{tag}/{i}/{k}"]
        if tag == "mlm":
            lab = g("txt_labels")
            out.append(dict(txt_labels=lab, scores=mlm_scripted_scores(int(g("seed")), lab[lab != -1])))
        elif tag in ("sap", "sapnan"):
            out.append(dict(scores=g("scores"), ob_action_viewindex=g("labels")))
        elif tag == "itm":
            out.append(dict(scores=g("scores"), labels=np.zeros(len(g("scores")), dtype=np.int64)))
        elif tag == "mrc":
            out.append(dict(scores=g("scores"), targets=g("targets"), hist_mrc_masks=g("hist_mrc_masks")))
        elif tag == "sar":
            out.append(dict(scores=g("scores"), ob_action_angles=g("ob_action_angles"), ob_progress=g("ob_progress")))
        else:
            out.append(dict(scores=g("scores"), sp_targets=g("sp_targets")))
    return out


def golden_f64(store, tag):
    """the pass of `tag` restated in float64 -> (values, exact, bound, ref_slack): the returned keys' values; which of them are exact
    (accuracies); per loss key the kernels' summed per-row bound after the normalisation; and per loss key what the REFERENCE's own
    arithmetic may add -- its per-batch fp32 reduction='sum' over n terms, n eps32 sum |term|, on top of the same per-row bound"""
    kind, bs = GOLDEN_TAGS[tag], golden_batches(store, tag)
    if kind in ("ce", "kl"):
        total = correct = n = bound = slack = 0
        for b in bs:
            if kind == "ce":
                lab = b["txt_labels"][b["txt_labels"] != -1] if tag == "mlm" else b.get("ob_action_viewindex", b.get("labels"))
                s, k, m, bd = eval_ce_f64(b["scores"], b["scores"].shape[1], lab)
                rows = ce_f64(b["scores"], lab)[0]
            else:
                s, k, m, bd = eval_kl_f64(b["scores"], b["targets"])
                rows = kl_f64(b["scores"], b["targets"])[0]
                slack += b["scores"].size * EPS32 * float(np.abs(rows).sum())        # kl_div sums R C elements, not R rows
            total, correct, n, bound = total + s, correct + k, n + m, bound + bd
            with np.errstate(invalid="ignore"):
                slack += len(rows) * EPS32 * float(np.abs(rows[np.isfinite(rows)]).sum())
        return ({"loss": total / n, "acc": correct / n, "n": n, "n_correct": correct}, ("acc", "n", "n_correct"),
                {"loss": bound / n}, {"loss": (bound + slack) / n})
    sums, n, slack = np.zeros(4), 0, np.zeros(4)
    for b in bs:
        x = b["scores"]
        if tag == "sar":
            t = np.concatenate([b["ob_action_angles"], b["ob_progress"][:, None]], axis=1)
        else:
            t = b["sp_targets"]
        if x.ndim == 3:                                            # main_r2r.py:437-438 on [B, 36, 2]: VIEW j, both components
            x, t = x[:, :2].transpose(1, 0, 2).reshape(2, -1).T, t[:, :2].transpose(1, 0, 2).reshape(2, -1).T
        s = eval_mse_cols_f64(x, t)
        sums[:len(s)] += s
        slack[:len(s)] += x.shape[0] * EPS32 * s
        n += b["scores"].shape[0]
    keys = ("heading_loss", "elevation_loss", "progress_loss")[:3 if tag == "sar" else 2]
    return ({k: sums[j] / n for j, k in enumerate(keys)} | {"n": n}, ("n",), {k: 1e-12 * sums[j] / n for j, k in enumerate(keys)},
            {k: (1e-12 * sums[j] + slack[j]) / n for j, k in enumerate(keys)})
