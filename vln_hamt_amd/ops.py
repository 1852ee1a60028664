"""autograd Functions over the C-ABI of libhamt_hip.so.

Every Function's forward and backward are HIP kernel launches on torch's *current* stream (raw
pointers + hipStream_t through ctypes); torch only owns the memory and the autograd graph.
There is no CPU or eager-PyTorch fallback: tensors must live on an AMD GPU and the library must load.

Precision: ``prec`` is ``"bf16"`` (bf16 MFMA operands, fp32 accumulate/epilogue; activations stay
fp32 in HBM and are rounded while staged) or ``"fp32"`` (exact fp32 MFMA).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import torch

from . import _lib as L

# ------------------------------------------------------------------------------------------ plumbing
_rng_state = {}
_call_counter = [0]


def rng_state(device) -> torch.Tensor:
    """Per-device dropout RNG words [seed, epoch] (uint64 stored as int64)."""
    d = torch.device(device)
    key = d.index
    if key is None:                      # "cuda" without an index means the CURRENT device (cuda:LOCAL_RANK), not cuda:0
        key = torch.cuda.current_device() if d.type == "cuda" else 0
    t = _rng_state.get(key)
    if t is None:
        t = torch.tensor([0x243F6A8885A308D3 & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64,
                         device=torch.device(d.type, key) if d.type == "cuda" else d)
        _rng_state[key] = t
    return t


def manual_seed(seed: int, device="cuda"):
    rng_state(device).copy_(torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64))
    _call_counter[0] = 0


def advance_rng_epoch(device="cuda"):
    """New dropout epoch (one kernel; graph-capturable).  Call once per optimisation step."""
    st = rng_state(device)
    L.check(L.load().hamt_rng_advance(_p(st), _stream()), "hamt_rng_advance")


def next_call_id() -> int:
    _call_counter[0] = (_call_counter[0] + 1) & 0xFFFFFFFF
    return _call_counter[0]


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise L.HamtError(f"{name}: tensor is on {t.device}; the HAMT kernels run on the GPU only (no CPU fallback)")


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.HAMT_F32
    if t.dtype == torch.bfloat16:
        return L.HAMT_BF16
    if t.dtype == torch.float16:     # IEEE half: `C` of a dense layer in front of a LayerNorm (hamt.h: HAMT_F16) -- hamt_gemm refuses it elsewhere
        return L.HAMT_F16
    if t.dtype == torch.uint8:       # the one-byte gelu' image (hamt.h: HAMT_U8G) -- `aux` of EPI_GELU_GRAD / EPI_MUL_AUX only
        return L.HAMT_U8G
    raise L.HamtError(f"unsupported dtype {t.dtype}")


def _prec(prec: str) -> int:
    return L.PREC_F32 if prec == "fp32" else L.PREC_BF16


def _ld(t: torch.Tensor) -> int:
    """Leading dimension (elements) of a 2-D row-major view whose last dim is contiguous."""
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), (t.shape, t.stride())
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _pad_cols(n: int, elem_size: int) -> int:
    q = 16 // elem_size
    return (n + q - 1) // q * q


def empty_rows(M: int, N: int, device, dtype=torch.float32) -> torch.Tensor:
    """[M,N] view whose rows start 16-byte aligned (row stride padded), e.g. the 30522-wide MLM logits."""
    return torch.empty(M, _pad_cols(N, torch.empty((), dtype=dtype).element_size()), dtype=dtype, device=device)[:, :N]


def _operand(t: torch.Tensor) -> torch.Tensor:
    """Return `t` if it satisfies the GEMM operand contract (unit inner stride, 16-byte aligned rows and
    base); otherwise a padded copy (only skinny / odd-width tensors such as [M,1] head gradients)."""
    es = t.element_size()
    ok = (t.stride(1) == 1 or t.shape[1] == 1) and t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or (t.stride(0) * es) % 16 == 0)
    if ok and not (t.shape[0] <= 1 and (t.shape[1] * es) % 16):
        return t
    o = empty_rows(t.shape[0], t.shape[1], t.device, t.dtype)
    o.copy_(t)
    return o


# ------------------------------------------------------------------------------------------ raw GEMM
def gemm(a, b, out, *, a_kmajor=False, b_kmajor=False, bias=None, epilogue=0, aux=None, prec="bf16", alpha=1.0,
         k_red=None, drop=None, k_valid=None):
    """out[M,N] = epi(alpha * op(a) @ op(b)); 2-D views with unit inner stride (strided rows allowed).
    drop = (p, call_id): HAMT_EPI_DROPOUT on the epilogue value (before the residual add).
    k_valid (K-strided operands: the weight-gradient form): only the first k_valid reduction rows count, the rest is padding of any
    content (the kernels re-read the last valid row instead and zero its products)."""
    _chk(a, "gemm")
    a, b = _operand(a), _operand(b)
    M, N = out.shape
    # reduction length: K-contiguous operands define it; K-strided operands may store fewer rows (ka/kb_rows)
    ka = a.shape[0] if a_kmajor else a.shape[1]
    kb = b.shape[0] if b_kmajor else b.shape[1]
    K = k_red if k_red is not None else max(ka, kb)
    assert (a.shape[1] == M if a_kmajor else a.shape == (M, K)), (a.shape, out.shape, K)
    assert (b.shape[1] == N if b_kmajor else b.shape == (N, K)), (b.shape, out.shape, K)
    assert ka <= K and kb <= K and (a_kmajor or ka == K) and (b_kmajor or kb == K)
    if _prec(prec) == L.PREC_F32:
        assert a.dtype == torch.float32 and b.dtype == torch.float32
    d = L.GemmDesc(M, N, K, _ld(a), _ld(b), _ld(out), _ld(aux) if aux is not None else 0, int(a_kmajor), int(b_kmajor),
                   _dt(a), _dt(b), _dt(out), _dt(aux) if aux is not None else 0, _prec(prec),
                   epilogue | (L.EPI_BIAS if bias is not None else 0), alpha, ka if ka < K else 0, kb if kb < K else 0, 0.0, 0, None)
    if k_valid is not None and k_valid < K:
        assert a_kmajor and b_kmajor and 0 < k_valid
        d.ka_rows, d.kb_rows = min(ka, k_valid), min(kb, k_valid)
    if drop is not None and drop[0] > 0.0:
        d.epilogue |= L.EPI_DROPOUT
        d.p_drop, d.call_id, d.rng = float(drop[0]), int(drop[1]), rng_state(out.device).data_ptr()
    lib = L.load()
    ks = 1
    if a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16:
        ks = lib.hamt_gemm_ksplit(C.byref(d))
    if ks > 1:      # deterministic split-K: fp32 partial tiles in a scratch buffer, summed in slice order
        ws = torch.empty(ks * M * N, dtype=torch.float32, device=out.device)
        L.check(lib.hamt_gemm_ws(C.byref(d), _p(a), _p(b), _p(out), _p(bias), _p(aux), _p(ws), ws.numel() * 4, _stream()), "hamt_gemm_ws")
    else:
        L.check(lib.hamt_gemm(C.byref(d), _p(a), _p(b), _p(out), _p(bias), _p(aux), _stream()), "hamt_gemm")
    return out


def colsum(x2d: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate=False) -> torch.Tensor:
    M, N = x2d.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x2d.device)
    ws = torch.empty(L.workspace_bytes(L.WS_COLSUM, M, N) // 4, dtype=torch.float32, device=x2d.device)
    L.check(L.load().hamt_colsum(M, N, _p(x2d), _ld(x2d), _dt(x2d), _p(out), int(accumulate), _p(ws), _stream()), "hamt_colsum")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    L.check(L.load().hamt_cast_f32_bf16(x.numel(), _p(x), _p(y), _stream()), "hamt_cast_f32_bf16")
    return y


def arena16_valid(w: torch.Tensor, a) -> bool:
    """Is the optimizer's bf16 shadow `a` (= w._hamt_arena16) still the image of `w`?  The arena's version counter moves
    with the optimizer's own updates; an in-place write to the parameter itself (load_state_dict, p.data.copy_, re-init:
    `p.data` is a view of the arena with its OWN version counter) moves only the parameter's, so both are compared."""
    return a[1]._version == a[2] and w._version == a[3] and a[1].data_ptr() <= w.data_ptr() < a[1].data_ptr() + a[1].numel() * 4


def weight_operand(w: torch.Tensor, prec: str) -> torch.Tensor:
    """GEMM B-operand for a parameter: fp32 master in fp32 mode, cached bf16 shadow in bf16 mode.
    The shadow is refreshed when the parameter's version counter or storage changes."""
    wd = w.detach()
    if prec == "fp32":
        return wd
    a = getattr(w, "_hamt_arena16", None)       # (bf16 view, fp32 arena, arena version, parameter version at last sync): optim.ArenaOptimizer
    if a is not None and arena16_valid(w, a):
        return a[0]
    c = getattr(w, "_hamt_w16", None)
    key = (w._version, _cache_epoch[0])
    if c is None or c[0] != key or c[1] != w.data_ptr():
        c = (key, w.data_ptr(), cast_bf16(wd)) + _cache_stamp(w)
        try:
            w._hamt_w16 = c
        except Exception:
            pass
    _cache_sync(c)
    return c[2]


ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


# ---- operand preparation for the bf16 fast GEMM (both operands bf16, K-contiguous, K % 64 == 0)
def _rup(n: int, m: int = 64) -> int:
    return (n + m - 1) // m * m


def cast_pad16(x2: torch.Tensor, cpad: Optional[int] = None, rpad: Optional[int] = None) -> torch.Tensor:
    """fp32 [R,C] (strided rows ok) -> bf16 [Rpad,Cpad], padding rows/columns zero-filled (defaults: multiples of 64)."""
    R, Cc = x2.shape
    cpad = _rup(Cc) if cpad is None else cpad
    rpad = _rup(R) if rpad is None else rpad
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    y = torch.empty(rpad, cpad, dtype=torch.bfloat16, device=x2.device)
    L.check(L.load().hamt_cast_pad_bf16(R, Cc, rpad, cpad, _p(x2), _ld(x2), _p(y), cpad, _stream()), "hamt_cast_pad_bf16")
    return y


def cast_pad16_dropout(x2: torch.Tensor, p: float, call_id: int) -> torch.Tensor:
    """bf16 [Rpad,C] image of x2 * keep-mask of the HAMT_EPI_DROPOUT GEMM with the same call id (C % 8 == 0)."""
    R, Cc = x2.shape
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    y = torch.empty(_rup(R), Cc, dtype=torch.bfloat16, device=x2.device)
    L.check(L.load().hamt_cast_pad_bf16_dropout(R, Cc, y.shape[0], _p(x2), _ld(x2), _p(y), Cc, float(p), int(call_id),
                                                _p(rng_state(x2.device)), _stream()), "hamt_cast_pad_bf16_dropout")
    return y


def cast_t16(x2: torch.Tensor, rpad: Optional[int] = None) -> torch.Tensor:
    """[R,C] fp32/bf16 (strided rows ok) -> bf16 [C,Rpad] = x^T, zero-filled padding columns."""
    R, Cc = x2.shape
    rpad = _rup(R) if rpad is None else rpad
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    y = torch.empty(Cc, rpad, dtype=torch.bfloat16, device=x2.device)
    L.check(L.load().hamt_cast_transpose(R, Cc, _p(x2), _ld(x2), _dt(x2), _p(y), rpad, rpad, _stream()), "hamt_cast_transpose")
    return y


_cache_epoch = [0]


def _cache_stamp(w):
    """(event, stream handle) of the stream that just built a lazily cached weight image: another stream (the model runs
    independent branches on two, streams.py) waits for the event before its first read."""
    if not w.is_cuda:
        return (None, None)
    st = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(st)
    return (ev, st.cuda_stream)


def _cache_sync(c):
    if c[3] is not None:
        st = torch.cuda.current_stream()
        if st.cuda_stream != c[4]:
            st.wait_event(c[3])


def invalidate_weight_caches():
    """Force every lazily cached weight shadow to be rebuilt at its next use (call right before capturing a graph so
    that the rebuild kernels are part of the captured step)."""
    _cache_epoch[0] += 1


def weight_t16(w: torch.Tensor) -> torch.Tensor:
    """cached bf16 W^T [K, Npad64] of a [N,K] parameter (B operand of the dgrad dX = dY W in NT form)."""
    c = getattr(w, "_hamt_wt16", None)
    key = (w._version, _cache_epoch[0])
    if c is None or c[0] != key or c[1] != w.data_ptr():
        c = (key, w.data_ptr(), cast_t16(w.detach())) + _cache_stamp(w)
        try:
            w._hamt_wt16 = c
        except Exception:
            pass
    _cache_sync(c)
    return c[2]


def _fast_ok(K: int) -> bool:
    return K % 64 == 0 and K >= 64


def prep_x16(x2: torch.Tensor, prec: str):
    """bf16 operand image of the activations [M,K] for the fast GEMMs: rows padded to a multiple of 64 with zeros so
    the same buffer serves as A of the forward (first M rows) and as the K-strided B of the weight gradient."""
    if prec != "bf16" or not _fast_ok(x2.shape[1]):
        return None
    if x2.dtype == torch.bfloat16 and x2.shape[0] % 64 == 0 and x2.is_contiguous():
        return x2
    assert x2.dtype == torch.float32
    return cast_pad16(x2, x2.shape[1])


def _linear_fwd(x2, weight, bias, out, act, prec, pre=None, x16=None):
    """out = act(x2 @ W^T + b).  bf16 mode with K % 64 == 0: x is cast once (x16 may be passed in to share it) and the
    GEMM takes the glds fast path; otherwise the generic kernel converts while staging."""
    epi = 0
    if act == ACT_GELU:
        epi |= L.EPI_GELU | (L.EPI_SAVE_PRE if pre is not None else 0)
    elif act == ACT_RELU:
        epi |= L.EPI_RELU
    a = x16[:x2.shape[0]] if x16 is not None else x2
    gemm(a, weight_operand(weight, prec), out, bias=bias, epilogue=epi, aux=pre if act == ACT_GELU else None, prec=prec)


def _linear_bwd(dy2, x2, x16, weight, prec, need_dx, need_dw, need_db, dx_out=None, dx_accumulate=False, dy16=None,
                bias_param=False):
    """dy2 [M,N] (strided rows ok), x [M,K] (x16 = its padded bf16 image or None), weight [N,K] parameter
    -> (dx [M,K], dW [N,K], db [N]); `bias_param` = the bias parameter (or None) enables queueing dW/db (wgrad.py), in
    which case dW and db come back as None.  bf16 mode: ONE padded bf16 image of dY feeds both contractions of the fast kernel:
    dX = dY16[M,Np] * W16 (W k-strided, "NN"), dW = dY16^T * X16 (both k-strided, "TN") -- no transposed copies."""
    M, N = dy2.shape
    K = weight.shape[1]
    dx = dw = db = None
    fast = prec == "bf16" and x16 is not None and N >= 8
    if fast and dy16 is None:
        dy16 = cast_pad16(dy2)                                   # [Mp, Np], zero padded
    if need_dx:
        dx = dx_out if dx_out is not None else torch.empty(M, K, dtype=torch.float32, device=dy2.device)
        epi = L.EPI_ACCUM if dx_accumulate else 0
        if fast:
            gemm(dy16[:M], weight_operand(weight, prec), dx, b_kmajor=True, epilogue=epi, prec=prec, k_red=dy16.shape[1])
        else:
            gemm(dy2, weight_operand(weight, prec), dx, b_kmajor=True, epilogue=epi, prec=prec)
    if need_dw and fast and bias_param is not False:
        from . import wgrad
        if wgrad.eligible(weight, dy16[:, :N], x16):    # queued for the grouped end-of-pass launch (wgrad.py); db rides along
            wgrad.defer(weight, bias_param if need_db else None, dy16[:, :N], x16)
            return dx, None, None
    slot_w = _accum_slot(weight) if (need_dw and not (K <= 8)) else None
    if slot_w is not None:
        # a parameter outside the grouped launch (the fp32 prediction heads) that owns a zero-at-the-start-of-a-step slot in the
        # optimizer's gradient arena: ADD dW (and db) there -- no autograd tensor for optim.ArenaOptimizer._pack_grads to copy in afterwards
        from . import wgrad
        wgrad.queue(dy2.device).current()
        if fast:
            gemm(dy16[:, :N], x16, slot_w, a_kmajor=True, b_kmajor=True, prec=prec, epilogue=L.EPI_ACCUM)
        else:
            gemm(dy2, x2 if x2 is not None else x16[:M], slot_w, a_kmajor=True, b_kmajor=True, prec=prec, epilogue=L.EPI_ACCUM)
        wgrad.publish_slot_grad(weight, slot_w)
        need_dw = False
        slot_b = _accum_slot(bias_param) if (need_db and torch.is_tensor(bias_param)) else None
        if slot_b is not None:
            colsum(dy2, out=slot_b, accumulate=True)
            wgrad.publish_slot_grad(bias_param, slot_b)
            need_db = False
    if need_dw:
        dw = torch.empty(N, K, dtype=torch.float32, device=dy2.device)
        if fast:
            gemm(dy16[:, :N], x16, dw, a_kmajor=True, b_kmajor=True, prec=prec)
        elif K <= 8 and x2 is not None and dy2.dtype == torch.float32 and x2.dtype == torch.float32:
            ws = torch.empty(64 * N * K, dtype=torch.float32, device=dy2.device)
            L.check(L.load().hamt_smallk_wgrad(M, N, K, _p(dy2), _ld(dy2), _p(x2), _ld(x2), _p(dw), 0, _p(ws), _stream()), "hamt_smallk_wgrad")
        else:
            gemm(dy2, x2 if x2 is not None else x16[:M], dw, a_kmajor=True, b_kmajor=True, prec=prec)
    if need_db:
        db = colsum(dy2)
    return dx, dw, db


SLOT_ACCUM = os.environ.get("HAMT_NO_SLOT_ACCUM") is None


def _accum_slot(p):
    """p's slot in the optimizer's flat gradient arena if a producer may ADD into it during this backward pass (a leaf parameter
    whose slot the update kernel leaves zero, inside a pass, .grad unset or already the slot), else None."""
    if p is None or not torch.is_tensor(p) or not p.is_leaf or not p.requires_grad or not SLOT_ACCUM:
        return None
    from . import wgrad
    slot = getattr(p, "_hamt_grad_slot", None)
    if (slot is None or not wgrad.ENABLED or torch._C._current_graph_task_id() < 0 or slot.shape != p.shape or not slot.is_contiguous()
            or not getattr(p, "_hamt_slot_zeroed", False) or not (p.grad is None or p.grad.data_ptr() == slot.data_ptr())):
        return None
    return slot


# ------------------------------------------------------------------------------------------ Linear
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b)  (nn.Linear + optional erf-GELU / ReLU; vilmodel.py:140, 168-171, 182, 263-264)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, prec, residual=None):
        _chk(x, "LinearFn")
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        N = weight.shape[0]
        M = x2.shape[0]
        x16 = prep_x16(x2, prec)
        # wide odd-width outputs (the 30522-column MLM logits) get a padded row stride so that they can feed the
        # backward GEMMs as 16-byte aligned operands; everything else is plain contiguous
        y = empty_rows(M, N, x.device) if (N % 4 and N >= 256) else torch.empty(M, N, dtype=torch.float32, device=x.device)
        pre = torch.empty(M, N, dtype=torch.float32, device=x.device) if act == ACT_GELU else None
        if residual is not None:                 # y = x W^T + b + residual in the GEMM epilogue (pre-LN residual add)
            assert act == ACT_NONE and residual.numel() == M * N
            r2 = residual.reshape(M, N)
            r2 = r2 if r2.is_contiguous() else r2.contiguous()
            a = x16[:M] if x16 is not None else x2
            gemm(a, weight_operand(weight, prec), y, bias=bias.detach() if bias is not None else None, epilogue=L.EPI_ADD_AUX,
                 aux=r2.detach(), prec=prec)
        else:
            _linear_fwd(x2, weight, bias.detach() if bias is not None else None, y, act, prec, pre, x16)
        # the bf16 image is all backward needs of x (weight gradient operand); keep fp32 x only on the generic path
        ctx.save_for_backward(x2 if x16 is None else None, x16, weight, pre if act == ACT_GELU else (y if act == ACT_RELU else None))
        ctx.act, ctx.prec, ctx.has_bias, ctx.xshape, ctx.M = act, prec, bias is not None, x.shape, M
        ctx.bias_param = bias if (bias is not None and bias.is_leaf) else (None if bias is None else False)
        ctx.res_shape = residual.shape if residual is not None else None
        return y if x.dim() == 2 else y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, x16, weight, h = ctx.saved_tensors
        N = weight.shape[0]
        dy2 = dy.reshape(-1, N)
        if ctx.act != ACT_NONE:
            dy2 = dy2.contiguous()
            h = h.contiguous()
            dh = torch.empty_like(dy2)
            L.check(L.load().hamt_act_bwd(dy2.numel(), _p(dy2), _p(h), ctx.act, _p(dh), _stream()), "hamt_act_bwd")
            dy2 = dh
        dy2 = _operand(dy2)
        dx, dw, db = _linear_bwd(dy2, x2, x16, weight, ctx.prec, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                 ctx.has_bias and ctx.needs_input_grad[2], bias_param=ctx.bias_param)
        dres = dy.reshape(ctx.res_shape) if (ctx.res_shape is not None and ctx.needs_input_grad[5]) else None
        return (dx.view(ctx.xshape) if dx is not None else None), dw, db, None, None, dres


def linear(x, weight, bias, act=ACT_NONE, prec="bf16", residual=None):
    """act(x W^T + b) (+ residual: added in the GEMM epilogue, act must be ACT_NONE)"""
    return LinearFn.apply(x, weight, bias, act, prec, residual)


class PackedLinearFn(torch.autograd.Function):
    """Several nn.Linear layers applied to the same input, written side by side into ONE packed buffer
    [M, sum(N_i)] (query/key/value of vilmodel.py:97-99 -> qkv; key/value of :324-325 -> kv) so the
    attention kernel reads heads by pointer arithmetic and no permute/contiguous copy is needed."""

    @staticmethod
    def forward(ctx, x, prec, *wb):
        _chk(x, "PackedLinearFn")
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        ws, bs = wb[0::2], wb[1::2]
        ns = [w.shape[0] for w in ws]
        out = torch.empty(x2.shape[0], sum(ns), dtype=torch.float32, device=x.device)
        x16 = prep_x16(x2, prec)
        c = 0
        for w, b, n in zip(ws, bs, ns):
            _linear_fwd(x2, w, b.detach(), out[:, c:c + n], ACT_NONE, prec, x16=x16)
            c += n
        ctx.save_for_backward(x2 if x16 is None else None, x16, *ws)
        ctx.prec, ctx.ns, ctx.xshape, ctx.M = prec, ns, x.shape, x2.shape[0]
        ctx.bias_params = [b if b.is_leaf else False for b in bs]
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, x16, *ws = ctx.saved_tensors
        dout = dout.contiguous()
        grads = []
        M = ctx.M
        K = ws[0].shape[1]
        dx = torch.empty(M, K, dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[0] else None
        fast = ctx.prec == "bf16" and x16 is not None and all(n % 64 == 0 for n in ctx.ns)
        d16 = cast_pad16(dout) if fast else None                  # [Mp, sum n]: column slices are the per-layer dY16
        c = 0
        for i, (w, n) in enumerate(zip(ws, ctx.ns)):
            _, dw, db = _linear_bwd(dout[:, c:c + n], x2, x16, w, ctx.prec, dx is not None, True, True, dx_out=dx,
                                    dx_accumulate=i > 0, dy16=d16[:, c:c + n] if fast else None, bias_param=ctx.bias_params[i])
            grads += [dw, db]
            c += n
        return (dx.view(ctx.xshape) if dx is not None else None), None, *grads


def packed_linear(x, prec, *linears):
    wb = []
    for lin in linears:
        wb += [lin.weight, lin.bias]
    return PackedLinearFn.apply(x, prec, *wb)


# ------------------------------------------------------------------------------------------ attention
class AttnFn(torch.autograd.Function):
    """softmax(Q K^T / sqrt(d) + mask) V with dropout on the probabilities (vilmodel.py:101-126, 327-348).
    `q_src` is either the packed self-attention buffer [B*S, 3H] (kv_src None) or the query projection
    [B*Sq, H] with `kv_src` = packed [B*Sk, 2H].  `add_mask` is the reference's additive (B,1,1,Sk) mask."""

    @staticmethod
    def forward(ctx, q_src, kv_src, add_mask, B, heads, p_drop, prec="fp32"):
        _chk(q_src, "AttnFn")
        packed = kv_src is None
        H = q_src.shape[1] // 3 if packed else q_src.shape[1]
        Sq = q_src.shape[0] // B
        if packed:
            q, k, v, Sk = q_src[:, :H], q_src[:, H:2 * H], q_src[:, 2 * H:], Sq
        else:
            q, k, v, Sk = q_src, kv_src[:, :H], kv_src[:, H:], kv_src.shape[0] // B
        mask2 = None
        if add_mask is not None:
            mask2 = add_mask.reshape(B, Sk).to(torch.float32).contiguous()
        out = torch.empty(B * Sq, H, dtype=torch.float32, device=q_src.device)
        lse = torch.empty(B * heads * Sq, dtype=torch.float32, device=q_src.device)
        cid = next_call_id()
        rng = rng_state(q_src.device)
        d = L.AttnDesc(B, heads, Sq, Sk, H // heads, _ld(q), _ld(k), _ld(v), H, _dt(q), L.HAMT_F32,
                       1.0 / math.sqrt(H // heads), float(p_drop), cid, _prec(prec))
        L.check(L.load().hamt_attn_small_fwd(C.byref(d), _p(q), _p(k), _p(v), _p(mask2), _p(out), _p(lse), _p(rng), _stream()),
                "hamt_attn_small_fwd")
        ctx.save_for_backward(q_src, kv_src, mask2, out, lse)
        ctx.desc_args = (B, heads, Sq, Sk, H, float(p_drop), cid, prec)
        return out

    @staticmethod
    def backward(ctx, dout):
        q_src, kv_src, mask2, out, lse = ctx.saved_tensors
        B, heads, Sq, Sk, H, p_drop, cid, prec = ctx.desc_args
        packed = kv_src is None
        dout = dout.contiguous()
        dq_src = torch.empty_like(q_src)
        dkv_src = None if packed else torch.empty_like(kv_src)
        if packed:
            q, k, v = q_src[:, :H], q_src[:, H:2 * H], q_src[:, 2 * H:]
            dq, dk, dv = dq_src[:, :H], dq_src[:, H:2 * H], dq_src[:, 2 * H:]
        else:
            q, k, v = q_src, kv_src[:, :H], kv_src[:, H:]
            dq, dk, dv = dq_src, dkv_src[:, :H], dkv_src[:, H:]
        d = L.AttnDesc(B, heads, Sq, Sk, H // heads, _ld(q), _ld(k), _ld(v), H, _dt(q), L.HAMT_F32,
                       1.0 / math.sqrt(H // heads), p_drop, cid, _prec(prec))
        L.check(L.load().hamt_attn_small_bwd(C.byref(d), _p(q), _p(k), _p(v), _p(mask2), _p(out), _p(dout), _p(lse), None,
                                             _p(dq), _p(dk), _p(dv), _p(rng_state(q_src.device)), _stream()),
                "hamt_attn_small_bwd")
        return dq_src, dkv_src, None, None, None, None, None


def attention(q_src, kv_src, add_mask, B, heads, p_drop, prec="fp32"):
    return AttnFn.apply(q_src, kv_src, add_mask, B, heads, p_drop, prec)


def attn_cls(q, k, v, heads: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(64)) v for ONE query per (image, head): q [n, heads*64], k / v [n*Sk, heads*64] (2-D views with unit inner
    stride, e.g. column blocks of a packed [k|v] buffer; fp32 or bf16, one dtype for the three) -> fp32 [n, heads*64].  Forward only
    (`hamt_attn_cls_fwd` keeps no log-sum-exp): refuses to run where autograd would record it."""
    _chk(q, "attn_cls")
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise L.HamtError("attn_cls: forward-only kernel (no backward); call it under torch.no_grad()")
    n, H = q.shape
    if H != heads * 64 or k.shape[1] != H or v.shape != k.shape or n == 0 or k.shape[0] % n or not (q.dtype == k.dtype == v.dtype):
        raise L.HamtError(f"attn_cls: q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)} {k.dtype}, v {tuple(v.shape)} {v.dtype}, heads {heads}")
    Sk = k.shape[0] // n
    out = torch.empty(n, H, dtype=torch.float32, device=q.device)
    d = L.AttnDesc(n, heads, 1, Sk, 64, _ld(q), _ld(k), _ld(v), H, _dt(q), L.HAMT_F32, 1.0 / math.sqrt(64), 0.0, 0, L.PREC_F32)
    L.check(L.load().hamt_attn_cls_fwd(C.byref(d), _p(q), _p(k), _p(v), _p(out), _stream()), "hamt_attn_cls_fwd")
    return out


# ------------------------------------------------------------------------------------------ LayerNorm family
def shadow16(x: torch.Tensor):
    """bf16 image [Mpad64, H] of an activation tensor if its producer emitted one (LayerNorm kernels do), else None."""
    s = getattr(x, "_hamt_bf16", None)
    if s is not None and s[1] == x._version and s[2] == x.data_ptr():
        return s[0]
    return None


LN_Z16 = os.environ.get("HAMT_LN_Z32") is None       # ablation: keep the saved pre-LN sum in fp32 behind a bf16 dense output as well


def _ln_io(t, flag_bf16, flag_f16):
    return flag_bf16 if t.dtype == torch.bfloat16 else (flag_f16 if t.dtype == torch.float16 else 0)


def _ln_fwd(x2, r2, gamma, beta, eps, p_pre, p_post, want16):
    """`x2` may be bf16 (the fused blocks' dense outputs in bf16 mode: what a linear returns under autocast); the pre-LN sum
    saved for backward is then kept in bf16 too (backward re-normalises it with the exact fp32 mean / rstd): 14 instead of
    18 bytes per element through this kernel, 14 instead of 16 through its backward."""
    M, H = x2.shape
    dev = x2.device
    x16_in = x2.dtype in (torch.bfloat16, torch.float16)
    # (the saved pre-LN sum takes the dense output's 2-byte format: half behind a half output -- |z| is O(1 .. 100) --, bf16 behind bf16)
    z = torch.empty(M, H, dtype=x2.dtype if (x16_in and LN_Z16) else torch.float32, device=dev)
    y = torch.empty(M, H, dtype=torch.float32, device=dev)
    mean = torch.empty(M, dtype=torch.float32, device=dev)
    rstd = torch.empty(M, dtype=torch.float32, device=dev)
    Mp = _rup(M) if want16 else 0
    y16 = torch.empty(Mp, H, dtype=torch.bfloat16, device=dev) if want16 else None
    cid = next_call_id() if (p_pre > 0 or p_post > 0) else 0
    d = L.LnDesc(M, H, float(eps), float(p_pre), float(p_post), cid, Mp, _ln_io(x2, L.LN_X_BF16, L.LN_X_F16) | _ln_io(z, L.LN_Z_BF16, L.LN_Z_F16))
    L.check(L.load().hamt_ln_fwd(C.byref(d), _p(x2), _p(r2), _p(gamma), _p(beta), _p(z), _p(y), _p(y16),
                                 _p(mean), _p(rstd), _p(rng_state(dev)), _stream()), "hamt_ln_fwd")
    return y, y16, z, mean, rstd, cid


LN_DEFER = os.environ.get("HAMT_NO_DEFER_LNRED") is None      # ablation: reduce the parameter-gradient partials in line


def _defer_ln_reduce(M, H, ws, red, want_dxsum, params, dev):
    """The partials are in `ws`: queue their summation for the ONE grouped launch at the end of the pass (wgrad.flush) and
    the publication of the results as the parameters' gradients."""
    from . import wgrad
    gamma_p, beta_p, bias_p = params
    wgrad.defer_ln_reduce(ws, red, M, H, want_dxsum, [(gamma_p, red[0]), (beta_p, red[1]), (bias_p, red[2] if want_dxsum else None)])


def _can_defer_ln(params, dev, H=64):
    from . import wgrad
    if not (LN_DEFER and wgrad.ENABLED and params is not None and dev.type == "cuda" and H % 64 == 0):
        return False
    return all(p is None or (isinstance(p, torch.Tensor) and p.is_leaf) for p in params)


def _ln_bwd(dy2, z, mean, rstd, gamma, eps, p_pre, p_post, cid, want_dx32, want_dx16, want_dxsum, params=None, dx16_out=None):
    """-> (dz, dx32 | None, dx16 | None, dgamma, dbeta, dxsum | None).  `params` = (gamma, beta, bias) PARAMETERS (bias:
    of the dense layer whose output fed the LayerNorm, or None): the per-block partials of their gradients are then
    summed by ONE grouped launch at the end of the pass (54 tiny reductions leave the critical path of a step), published
    there as `.grad` (wgrad.defer_ln_reduce) and returned as None here."""
    M, H = dy2.shape
    dev = dy2.device
    dz = torch.empty(M, H, dtype=torch.float32, device=dev)
    dx = torch.empty(M, H, dtype=torch.float32, device=dev) if (want_dx32 and p_pre > 0) else None
    Mp = _rup(M) if want_dx16 else 0
    if dx16_out is not None:      # caller-provided rows of a larger bf16 image
        assert want_dx16 and dx16_out.shape == (Mp, H) and dx16_out.is_contiguous()
        dx16 = dx16_out
    else:
        dx16 = torch.empty(Mp, H, dtype=torch.bfloat16, device=dev) if want_dx16 else None
    red = torch.empty(3, H, dtype=torch.float32, device=dev)      # stored (not accumulated) by the reduce kernel
    ws = torch.empty(L.workspace_bytes(L.WS_LN_BWD, M, H) // 4, dtype=torch.float32, device=dev)
    d = L.LnDesc(M, H, float(eps), float(p_pre), float(p_post), cid, Mp, _ln_io(z, L.LN_Z_BF16, L.LN_Z_F16))
    defer = _can_defer_ln(params, dev, H)
    L.check(L.load().hamt_ln_bwd(C.byref(d), _p(dy2), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dz), _p(dx), _p(dx16),
                                 None if defer else _p(red[0]), None if defer else _p(red[1]),
                                 _p(red[2]) if (want_dxsum and not defer) else None, _p(ws), _p(rng_state(dev)), _stream()),
            "hamt_ln_bwd")
    if defer:
        _defer_ln_reduce(M, H, ws, red, want_dxsum, params, dev)
        return dz, dx, dx16, None, None, None
    return dz, dx, dx16, red[0], red[1], (red[2] if want_dxsum else None)


class LnFn(torch.autograd.Function):
    """y = dropout_post(LayerNorm(dropout_pre(x) + residual)) -- see hamt_ln_fwd in include/hamt.h.
    Second output: the bf16 image of y (rows padded to a multiple of 64) for the next GEMM, or None."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, p_pre, p_post, want16):
        _chk(x, "LnFn")
        H = x.shape[-1]
        x2 = x.reshape(-1, H).contiguous()
        r2 = residual.reshape(-1, H).contiguous() if residual is not None else None
        y, y16, z, mean, rstd, cid = _ln_fwd(x2, r2, gamma.detach(), beta.detach(), eps, p_pre, p_post, want16)
        ctx.save_for_backward(z, mean, rstd, gamma)
        ctx.ln_params = (gamma, beta, None)
        ctx.args = (float(eps), float(p_pre), float(p_post), cid, residual is not None, x.shape)
        if y16 is not None:
            ctx.mark_non_differentiable(y16)
        ctx.set_materialize_grads(False)         # no zero-filled stand-in for the bf16 image's (non-existent) gradient
        return y.view(x.shape), y16

    @staticmethod
    def backward(ctx, dy, _d16=None):
        if dy is None:
            return (None,) * 8
        z, mean, rstd, gamma = ctx.saved_tensors
        eps, p_pre, p_post, cid, has_res, xshape = ctx.args
        dy2 = dy.reshape(z.shape).contiguous()
        dz, dx, _, dgamma, dbeta, _ = _ln_bwd(dy2, z, mean, rstd, gamma.detach(), eps, p_pre, p_post, cid, True, False, False,
                                              params=ctx.ln_params)
        gx = (dx if dx is not None else dz).view(xshape)
        return gx, (dz.view(xshape) if has_res else None), dgamma, dbeta, None, None, None, None


def layer_norm(x, residual, ln_module, p_pre=0.0, p_post=0.0, eps=None, want16=False):
    y, y16 = LnFn.apply(x, residual, ln_module.weight, ln_module.bias, ln_module.eps if eps is None else eps, p_pre, p_post, want16)
    if y16 is not None:
        y._hamt_bf16 = (y16, y._version, y.data_ptr())
    return y


# ------------------------------------------------------------------------------------------ two-stream visual embedding
VIS_EMBED = os.environ.get("HAMT_VIS_EMBED", "1") == "1"
# bf16 dense output in front of the fused kernel (-6 us per step at B = 64): OFF -- the history embedder is where ITM's candidates
# differ, and its logits sit at 0.9 of the 1e-2 parity bound already (1.02e-2 on one canon_ragged draw with this on)
VIS_EMBED_X16 = os.environ.get("HAMT_VIS_EMBED_X16", "0") == "1"


SLOT_ACCUM_VE = os.environ.get("HAMT_VIS_EMBED_NO_SLOT") is None


def _grad_dst(p, shape, dev, in_pass):
    """-> (tensor the kernel ADDS p's gradient to, what backward returns for p): p's slot in the optimizer's gradient arena (zero at
    the start of a step; published as `.grad` at the end of the pass, as ops.GatherRowsFn does) or a fresh zero tensor."""
    slot = getattr(p, "_hamt_grad_slot", None) if (in_pass and p is not None and p.is_leaf and p.requires_grad and SLOT_ACCUM_VE) else None
    if (slot is not None and slot.shape == p.shape and slot.is_contiguous() and getattr(p, "_hamt_slot_zeroed", False)
            and (p.grad is None or p.grad.data_ptr() == slot.data_ptr())):
        return slot, None
    t = torch.zeros(shape, dtype=torch.float32, device=dev)
    return t, t


class VisEmbedFn(torch.autograd.Function):
    """e = img_layer_norm(img_linear(img)) + ang_layer_norm(ang_linear(ang))  (vilmodel.py:498-500, 549-551, 557-558): the dense
    layer, then ONE launch for the K = 4 angle projection, both LayerNorms and the sum
    (hamt_vis_embed_fwd; csrc/vis_embed.hip); backward one launch + a small reduction, the image stream's gradient leaving as
    the bf16 image img_linear's queued weight gradient reads.  Second output: the bf16 image of e (or None)."""

    @staticmethod
    def forward(ctx, img, ang, w1, b1, g1, be1, w2, b2, g2, be2, eps1, eps2, prec, want16):
        _chk(img, "VisEmbedFn")
        K, H, A = img.shape[-1], w1.shape[0], ang.shape[-1]
        x2 = img.reshape(-1, K)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        M = x2.shape[0]
        dev = img.device
        a2 = ang.reshape(M, A).to(torch.float32).contiguous()
        x16 = prep_x16(x2, prec)
        x1 = torch.empty(M, H, dtype=torch.bfloat16 if (x16 is not None and VIS_EMBED_X16) else torch.float32, device=dev)
        _linear_fwd(x2, w1, b1.detach() if b1 is not None else None, x1, ACT_NONE, prec, None, x16)
        y = torch.empty(M, H, dtype=torch.float32, device=dev)
        Mp = _rup(M) if want16 else 0
        y16 = torch.empty(Mp, H, dtype=torch.bfloat16, device=dev) if want16 else None
        stats = torch.empty(4, M, dtype=torch.float32, device=dev)
        d = L.VisEmbedDesc(M, H, A, A, float(eps1), float(eps2), int(x1.dtype == torch.bfloat16), Mp)
        L.check(L.load().hamt_vis_embed_fwd(C.byref(d), _p(x1), _p(a2), _p(w2.detach()), _p(b2.detach()), _p(g1.detach()), _p(be1.detach()),
                                            _p(g2.detach()), _p(be2.detach()), _p(y), _p(y16), _p(stats), _stream()), "hamt_vis_embed_fwd")
        ctx.save_for_backward(x2 if x16 is None else None, x16, x1, a2, stats, w1, g1, w2, b2, g2)
        ctx.params = (g1, be1, g2, be2, b2, w2)
        ctx.args = (float(eps1), float(eps2), prec, img.shape, b1 is not None)
        ctx.bias_param = b1 if (b1 is not None and b1.is_leaf) else (None if b1 is None else False)
        if y16 is not None:
            ctx.mark_non_differentiable(y16)
        ctx.set_materialize_grads(False)
        return y.view(*img.shape[:-1], H), y16

    @staticmethod
    def backward(ctx, dy, _d16=None):
        if dy is None:
            return (None,) * 14
        x2, x16, x1, a2, stats, w1, g1, w2, b2, g2 = ctx.saved_tensors
        eps1, eps2, prec, ishape, has_b1 = ctx.args
        M, H = x1.shape
        A = a2.shape[1]
        dev = dy.device
        dy2 = dy.reshape(M, H).contiguous()
        from . import wgrad
        in_pass = wgrad.ENABLED and torch._C._current_graph_task_id() >= 0
        fast = x16 is not None
        Mp = _rup(M) if fast else 0
        dx16 = torch.empty(Mp, H, dtype=torch.bfloat16, device=dev) if fast else None
        dx = None if fast else torch.empty(M, H, dtype=torch.float32, device=dev)
        dst = [_grad_dst(p, p.shape, dev, in_pass) if ctx.needs_input_grad[i] else (None, None)
               for p, i in zip(ctx.params, (4, 5, 8, 9, 7, 6))]          # gamma_img, beta_img, gamma_ang, beta_ang, b_ang, w_ang
        scratch = [None if t is not None else torch.zeros(p.shape, dtype=torch.float32, device=dev) for (t, _), p in zip(dst, ctx.params)]
        out = [t if t is not None else s_ for (t, _), s_ in zip(dst, scratch)]
        if any(t is not None and r is None for t, r in dst):
            wgrad.queue(dev).current()              # (opens the pass: orders this stream behind an overlapped optimizer update)
        ws = torch.empty(L.workspace_bytes(L.WS_VIS_EMBED_BWD, M, H) // 4, dtype=torch.float32, device=dev)
        d = L.VisEmbedDesc(M, H, A, A, eps1, eps2, int(x1.dtype == torch.bfloat16), Mp)
        L.check(L.load().hamt_vis_embed_bwd(C.byref(d), _p(dy2), _p(x1), _p(a2), _p(w2.detach()), _p(b2.detach()), _p(g1.detach()), _p(g2.detach()),
                                            _p(stats), _p(dx), _p(dx16), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(out[4]), _p(out[5]),
                                            _p(ws), _stream()), "hamt_vis_embed_bwd")
        for (t, r), p in zip(dst, ctx.params):
            if t is not None and r is None:
                wgrad.publish_slot_grad(p, t)
        rets = [r for _, r in dst]
        dimg, dw1, db1 = _linear_bwd(dx16[:M] if fast else dx, x2, x16, w1, prec, ctx.needs_input_grad[0], ctx.needs_input_grad[2],
                                     has_b1 and ctx.needs_input_grad[3], dy16=dx16, bias_param=ctx.bias_param)
        return ((dimg.view(ishape) if dimg is not None else None), None, dw1, db1, rets[0], rets[1], rets[5], rets[4], rets[2], rets[3],
                None, None, None, None)


def vis_embed_ok(img, ang, img_lin, ang_lin) -> bool:
    H = img_lin.weight.shape[0]
    return (VIS_EMBED and img.is_cuda and ang.shape[-1] == 4 and H % 64 == 0 and H <= 1024 and img.dtype == torch.float32
            and ang_lin.bias is not None and img_lin.weight.dtype == torch.float32)


def vis_embed(img, ang, img_lin, img_ln, ang_lin, ang_ln, prec, want16=False):
    y, y16 = VisEmbedFn.apply(img, ang, img_lin.weight, img_lin.bias, img_ln.weight, img_ln.bias, ang_lin.weight, ang_lin.bias,
                              ang_ln.weight, ang_ln.bias, img_ln.eps, ang_ln.eps, prec, want16)
    if y16 is not None:
        y._hamt_bf16 = (y16, y._version, y.data_ptr())
    return y


# ------------------------------------------------------------------------------------------ REVERIE object embedding
OBJ_EMBED = os.environ.get("HAMT_OBJ_EMBED", "1") == "1"
# bf16 dense output in front of the fused kernel (bf16 mode): off by default, as HAMT_VIS_EMBED_X16
OBJ_EMBED_X16 = os.environ.get("HAMT_OBJ_EMBED_X16", "0") == "1"
_OE_GRAD_IN = (7, 8, 11, 12, 5, 6, 9, 10, 13, 14, 15, 16, 17, 18)   # hamt_obj_embed_grads field i <- ObjEmbedFn input _OE_GRAD_IN[i]
_OE_ROW = {15: 1, 16: 2}                                              # token_type row 1, nav_type row 2 (the STOP type)


def _rows_view(t: torch.Tensor, M: int, W: int) -> torch.Tensor:
    """[..., W] fp32 -> [M, W] with unit inner stride (any row stride: the agent's angle slices of a wider feature tensor)"""
    t2 = t.reshape(M, W) if t.dtype == torch.float32 else t.to(torch.float32).reshape(M, W)
    return t2 if (t2.stride(-1) == 1 and (M <= 1 or t2.stride(0) >= W)) else t2.contiguous()


class ObjEmbedFn(torch.autograd.Function):
    """y = dropout(LN_out(LN_img(img_linear(obj)) + LN_ang(ang_linear(ang)) + LN_pos(pos_linear(pos)) + nav[2] + tt[1]))
    (reverie/vlnbert_navref.py:31-42): the dense layer, then ONE launch for both small projections, the four LayerNorms, the two
    constant rows and the dropout (hamt_obj_embed_fwd; csrc/obj_embed.hip); backward one launch + a deterministic reduction, the
    image stream's gradient leaving as the bf16 image img_linear's queued weight gradient reads.  `tt` / `nav` are the whole
    token-type / navigation-type tables: their rows 1 / 2 receive colsum(d(LN_out input)), ADDED to whatever else those rows get."""

    @staticmethod
    def forward(ctx, obj, ang, pos, w1, b1, g_img, be_img, w_ang, b_ang, g_ang, be_ang, w_pos, b_pos, g_pos, be_pos, tt, nav,
                g_out, be_out, eps, p_drop, prec):
        _chk(obj, "ObjEmbedFn")
        K, H = obj.shape[-1], w1.shape[0]
        x2 = obj.reshape(-1, K)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        M = x2.shape[0]
        dev = obj.device
        a2, p2 = _rows_view(ang, M, ang.shape[-1]), _rows_view(pos, M, pos.shape[-1])
        x16 = prep_x16(x2, prec)
        x1 = torch.empty(M, H, dtype=torch.bfloat16 if (x16 is not None and OBJ_EMBED_X16) else torch.float32, device=dev)
        _linear_fwd(x2, w1, b1.detach() if b1 is not None else None, x1, ACT_NONE, prec, None, x16)
        y = torch.empty(M, H, dtype=torch.float32, device=dev)
        stats = torch.empty(8, M, dtype=torch.float32, device=dev)
        cid = next_call_id() if p_drop > 0 else 0
        d = L.ObjEmbedDesc(M, H, a2.shape[1], a2.stride(0), p2.shape[1], p2.stride(0), *[float(e) for e in eps], float(p_drop), cid,
                           int(x1.dtype == torch.bfloat16), 0)
        params = (w_ang, b_ang, w_pos, b_pos, g_img, be_img, g_ang, be_ang, g_pos, be_pos, tt, nav, g_out, be_out)
        pp = ObjEmbedFn._params(params, H)
        L.check(L.load().hamt_obj_embed_fwd(C.byref(d), C.byref(pp), _p(x1), _p(a2), _p(p2), _p(y), _p(stats), _p(rng_state(dev)), _stream()),
                "hamt_obj_embed_fwd")
        ctx.save_for_backward(x2 if x16 is None else None, x16, x1, a2, p2, stats, w1, *params)
        ctx.args = (tuple(float(e) for e in eps), float(p_drop), cid, prec, obj.shape, b1 is not None)
        ctx.bias_param = b1 if (b1 is not None and b1.is_leaf) else (None if b1 is None else False)
        ctx.grad_params = {i: p for i, p in zip(range(7, 19), (w_ang, b_ang, g_ang, be_ang, w_pos, b_pos, g_pos, be_pos, tt, nav, g_out, be_out))}
        ctx.grad_params.update({5: g_img, 6: be_img})
        ctx.set_materialize_grads(False)
        return y.view(*obj.shape[:-1], H)

    @staticmethod
    def _params(params, H):
        ptrs = []
        for name, t in zip(L.OBJ_EMBED_PARAMS, params):
            t = t.detach()
            assert t.is_contiguous() and t.dtype == torch.float32, name
            row = 1 if name == "tt" else (2 if name == "nav" else 0)
            ptrs.append(t.data_ptr() + row * H * 4)
        return L.ObjEmbedParams(*ptrs)

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 22
        x2, x16, x1, a2, p2, stats, w1, *params = ctx.saved_tensors
        eps, p_drop, cid, prec, oshape, has_b1 = ctx.args
        M, H = x1.shape
        dev = dy.device
        dy2 = dy.reshape(M, H).contiguous()
        from . import wgrad
        in_pass = wgrad.ENABLED and torch._C._current_graph_task_id() >= 0
        fast = x16 is not None
        Mp = _rup(M) if fast else 0
        dx16 = torch.empty(Mp, H, dtype=torch.bfloat16, device=dev) if fast else None
        dx = None if fast else torch.empty(M, H, dtype=torch.float32, device=dev)
        ptrs, rets = [], {}
        for i in _OE_GRAD_IN:
            if not ctx.needs_input_grad[i]:
                ptrs.append(None)
                continue
            p = ctx.grad_params[i]
            t, r = _grad_dst(p, p.shape, dev, in_pass)
            if r is None:
                wgrad.queue(dev).current()          # (opens the pass: orders this stream behind an overlapped optimizer update)
            rets[i] = (p, t, r)
            ptrs.append(t.data_ptr() + _OE_ROW.get(i, 0) * H * 4)
        g = L.ObjEmbedGrads(*ptrs)
        ws = torch.empty(L.workspace_bytes(L.WS_OBJ_EMBED_BWD, M, H) // 4, dtype=torch.float32, device=dev)
        d = L.ObjEmbedDesc(M, H, a2.shape[1], a2.stride(0), p2.shape[1], p2.stride(0), *eps, p_drop, cid, int(x1.dtype == torch.bfloat16), Mp)
        pp = ObjEmbedFn._params(params, H)
        L.check(L.load().hamt_obj_embed_bwd(C.byref(d), C.byref(pp), C.byref(g), _p(dy2), _p(x1), _p(a2), _p(p2), _p(stats), _p(dx), _p(dx16),
                                            _p(ws), _p(rng_state(dev)), _stream()), "hamt_obj_embed_bwd")
        out = [None] * 22
        for i, (p, t, r) in rets.items():
            if r is None:
                wgrad.publish_slot_grad(p, t)
            out[i] = r
        dobj, dw1, db1 = _linear_bwd(dx16[:M] if fast else dx, x2, x16, w1, prec, ctx.needs_input_grad[0], ctx.needs_input_grad[3],
                                     has_b1 and ctx.needs_input_grad[4], dy16=dx16, bias_param=ctx.bias_param)
        out[0] = dobj.view(oshape) if dobj is not None else None
        out[3], out[4] = dw1, db1
        return tuple(out)


def obj_embed_ok(obj, ang, pos, emb, tt, nav) -> bool:
    """the fused object embedder applies: fp32 features on the GPU, 4 angle / 5 position features, H % 64 == 0, H <= 1024, fp32
    16-byte aligned parameters (`emb` = the ObjectEmbeddings module, tt / nav = the token-type / navigation-type tables)"""
    H = emb.img_linear.weight.shape[0]
    if not (OBJ_EMBED and obj.is_cuda and obj.dtype == torch.float32 and ang.shape[-1] == 4 and pos.shape[-1] == 5
            and H % 64 == 0 and H <= 1024 and emb.ang_linear.bias is not None and emb.pos_linear.bias is not None):
        return False
    ts = [emb.ang_linear.weight, emb.ang_linear.bias, emb.pos_linear.weight, emb.pos_linear.bias, tt, nav]
    ts += [m.weight for m in (emb.img_layer_norm, emb.ang_layer_norm, emb.pos_layer_norm, emb.layer_norm)]
    ts += [m.bias for m in (emb.img_layer_norm, emb.ang_layer_norm, emb.pos_layer_norm, emb.layer_norm)]
    return (emb.img_linear.weight.dtype == torch.float32 and tt.shape[0] > 1 and nav.shape[0] > 2
            and all(t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts))


def obj_embed(obj, ang, pos, emb, tt, nav, p_drop, prec):
    """ObjEmbedFn over the parameters of an ObjectEmbeddings module `emb` (reverie/vlnbert_navref.py)"""
    il, al, pl = emb.img_linear, emb.ang_linear, emb.pos_linear
    n1, n2, n3, n4 = emb.img_layer_norm, emb.ang_layer_norm, emb.pos_layer_norm, emb.layer_norm
    return ObjEmbedFn.apply(obj, ang, pos, il.weight, il.bias, n1.weight, n1.bias, al.weight, al.bias, n2.weight, n2.bias, pl.weight, pl.bias,
                            n3.weight, n3.bias, tt, nav, n4.weight, n4.bias, (n1.eps, n2.eps, n3.eps, n4.eps), float(p_drop), prec)


# ------------------------------------------------------------------------------------------ gathers / embeddings
class EmbedSumFn(torch.autograd.Function):
    """word[ids] + position[:L] + token_type[0]  (vilmodel.py:62-66; int64 gather is bit exact)."""

    @staticmethod
    def forward(ctx, ids, word, pos, typ):
        _chk(word, "EmbedSumFn")
        B, Lq = ids.shape
        H = word.shape[1]
        ids = ids.contiguous()
        z = torch.empty(B, Lq, H, dtype=torch.float32, device=word.device)
        L.check(L.load().hamt_embed_sum_fwd(B, Lq, H, _p(ids), _p(word.detach()), _p(pos.detach()), _p(typ.detach()), _p(z), _stream()),
                "hamt_embed_sum_fwd")
        ctx.save_for_backward(ids)
        ctx.shapes = (word.shape, pos.shape, typ.shape)
        ctx.tables = (word, pos, typ)
        return z

    @staticmethod
    def backward(ctx, dz):
        (ids,) = ctx.saved_tensors
        B, Lq = ids.shape
        dz = dz.contiguous()
        H = dz.shape[-1]
        dev = dz.device
        from . import wgrad
        in_pass = wgrad.ENABLED and torch._C._current_graph_task_id() >= 0
        outs, rets = [], []
        for p, shape in zip(ctx.tables, ctx.shapes):
            # a table that owns a (zero at the start of a step) slot in the optimizer's gradient arena: add there -- no zero fill
            # of the 94 MB word table, no copy into the arena afterwards (as ops.GatherRowsFn does); published as `.grad` at the
            # end of the pass, the tied MLM decoder's queued weight gradient then accumulates on top
            slot = getattr(p, "_hamt_grad_slot", None) if (in_pass and p.is_leaf and p.requires_grad) else None
            if (slot is not None and slot.shape == p.shape and slot.is_contiguous() and getattr(p, "_hamt_slot_zeroed", False)
                    and (p.grad is None or p.grad.data_ptr() == slot.data_ptr())):
                outs.append(slot)
                rets.append(None)
            else:
                t = torch.zeros(shape, dtype=torch.float32, device=dev)
                outs.append(t)
                rets.append(t)
        dword, dpos, dtyp = outs
        if any(r is None for r in rets):
            wgrad.queue(dev).current()              # (opens the pass: orders this stream behind an overlapped optimizer update)
        ws = torch.empty(L.workspace_bytes(L.WS_EMBED_BWD, B * Lq, H) // 4, dtype=torch.float32, device=dev)
        L.check(L.load().hamt_embed_sum_bwd(B, Lq, H, dword.shape[0], _p(ids), _p(dz), _p(dword), _p(dpos), _p(dtyp), _p(ws), ws.numel() * 4, _stream()),
                "hamt_embed_sum_bwd")      # (dtyp: row 0 of the type table)
        for p, r, o in zip(ctx.tables, rets, outs):
            if r is None:
                wgrad.publish_slot_grad(p, o)
        return None, rets[0], rets[1], rets[2]


def _scatter_add(R, W, dout, idx, table, unique=False):
    """table[idx[r]] += dout[r] in a fixed summation order (bit-reproducible): tables of a few rows (token / navigability types, the cls
    token) by per-block partial sums (hamt_scatter_add_rows_small), larger ones (position tables, compaction scatters) by one writer per
    table row walking its colliding source rows in row order (hamt_scatter_add_rows_ordered)"""
    T = table.numel() // W
    if unique:        # no two source rows share a table row (a compaction / slice): every element is added once, order cannot matter
        L.check(L.load().hamt_scatter_add_rows(R, W, _p(dout), W, 0, _p(idx), _p(table), W, _stream()), "hamt_scatter_add_rows")
    elif T <= 8 and table.is_contiguous():
        ws = torch.empty(64 * T * W, dtype=torch.float32, device=dout.device)
        L.check(L.load().hamt_scatter_add_rows_small(R, W, _p(dout), W, 0, _p(idx), T, _p(table), _p(ws), _stream()), "hamt_scatter_add_rows_small")
    else:
        ws = torch.empty(34 * max(R, 1), dtype=torch.int32, device=dout.device)
        L.check(L.load().hamt_scatter_add_rows_ordered(R, W, _p(dout), W, 0, _p(idx), _p(table), W, T, _p(ws), _stream()), "hamt_scatter_add_rows_ordered")


class GatherRowsFn(torch.autograd.Function):
    """out[r] = (base[r] if base is not None else 0) + table[idx[r]]  over rows of width W.
    Serves embedding lookups, boolean-mask compaction, anchor gathers and slices (idx arithmetic)."""

    @staticmethod
    def forward(ctx, table, idx, base, unique=False):
        _chk(table, "GatherRowsFn")
        ctx.unique = bool(unique)
        W = table.shape[-1]
        t2 = table.reshape(-1, W)
        if t2.stride(-1) != 1:
            t2 = t2.contiguous()
        idx = idx.reshape(-1).contiguous()
        R = idx.numel()
        b2 = base.reshape(R, W).contiguous() if base is not None else None
        out = torch.empty(R, W, dtype=torch.float32, device=table.device)
        L.check(L.load().hamt_gather_rows(R, W, _p(t2.detach()), _ld(t2), _p(idx), _p(b2), W, _p(out), W, 0, _stream()),
                "hamt_gather_rows")
        ctx.save_for_backward(idx)
        ctx.tshape, ctx.has_base, ctx.bshape = table.shape, base is not None, (base.shape if base is not None else None)
        ctx.table_param = table if (table.is_leaf and table.requires_grad and getattr(table, "_hamt_grad_slot", None) is not None) else None
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        dout = dout.contiguous()
        R, W = dout.shape
        dtab = None
        if ctx.needs_input_grad[0]:
            p = ctx.table_param
            slot = getattr(p, "_hamt_grad_slot", None) if p is not None else None
            from . import wgrad
            if (slot is not None and wgrad.ENABLED and slot.shape == p.shape and slot.is_contiguous() and getattr(p, "_hamt_slot_zeroed", False)
                    and (p.grad is None or p.grad.data_ptr() == slot.data_ptr()) and torch._C._current_graph_task_id() >= 0):
                # an embedding table that owns a slot in the optimizer's gradient arena (zero at the start of a step): add the rows
                # there -- no 94 MB zero fill for the 30 522 x 768 word table, no copy into the arena afterwards; published as
                # `.grad` at the end of the pass (the tied MLM decoder's queued weight gradient then accumulates on top)
                wgrad.queue(slot.device).current()         # (opens the pass: orders this stream behind an overlapped optimizer update)
                _scatter_add(R, W, dout, idx, slot, ctx.unique)
                wgrad.publish_slot_grad(p, slot)
            else:
                dtab = torch.zeros(ctx.tshape, dtype=torch.float32, device=dout.device)
                _scatter_add(R, W, dout, idx, dtab, ctx.unique)
        return dtab, None, (dout.view(ctx.bshape) if ctx.has_base else None), None


def gather_rows(table, idx, base=None, unique=False):
    """unique: the caller guarantees that no index repeats (a compaction of masked positions, a slice, one row per sample): the
    backward then adds every gradient row to its own table row, where the order of the adds cannot matter"""
    return GatherRowsFn.apply(table, idx, base, unique)


_CONST_IDX: dict = {}


def const_index(kind: str, *args, device) -> torch.Tensor:
    """A constant int64 index tensor, built once per (kind, arguments, device) and never modified: `zeros` n / `ones` n / `arange` n
    (0 .. n-1) / `arange_mul` (n, k) = arange(n) * k / `bcast` (n_outer, n_inner) = row -> outer index / `rows_but_last` (B, S) = b * S +
    s for s < S - 1.  A forward pass used to rebuild these with 1-3 tiny fill / arange / multiply launches each, every step (and every
    replay of a captured step)."""
    key = (kind, args, str(torch.device(device)))
    t = _CONST_IDX.get(key)
    if t is None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():      # (first use inside a capture: no persistent memory there)
            return _build_const(kind, args, device)
        with torch.no_grad():
            t = _CONST_IDX[key] = _build_const(kind, args, device)
        if t.is_cuda:       # (once per constant: whichever stream uses it next finds it written)
            torch.cuda.current_stream(t.device).synchronize()
    return t


def _build_const(kind, args, device):
    if kind == "zeros":
        return torch.zeros(args[0], dtype=torch.long, device=device)
    if kind == "ones":
        return torch.ones(args[0], dtype=torch.long, device=device)
    if kind == "arange":
        return torch.arange(args[0], dtype=torch.long, device=device)
    if kind == "arange_mul":
        return torch.arange(args[0], dtype=torch.long, device=device) * args[1]
    if kind == "bcast":
        return torch.arange(args[0], device=device).repeat_interleave(args[1])
    if kind == "rows_but_last":
        B, S = args
        return (torch.arange(B, device=device)[:, None] * S + torch.arange(S - 1, device=device)[None]).reshape(-1)
    raise ValueError(kind)


@torch.no_grad()
def extend_mask(mask: torch.Tensor) -> torch.Tensor:
    """(B, S) bool keep-mask -> additive (B, 1, 1, S) fp32 = (1 - m) * -10000 (vilmodel.py:597-599) in one launch"""
    if mask.dtype != torch.bool or not mask.is_cuda:
        return (1.0 - mask[:, None, None, :].to(torch.float32)) * -10000.0
    m = mask.contiguous()
    out = torch.empty(m.shape[0], 1, 1, m.shape[1], dtype=torch.float32, device=m.device)
    L.check(L.load().hamt_extend_mask(m.numel(), _p(m), _p(out), _stream()), "hamt_extend_mask")
    return out


@torch.no_grad()
def copy_rows_into(dst2d: torch.Tensor, col0: int, src2d: torch.Tensor):
    """dst2d[:, col0:col0 + W] = src2d  (fp32, rows of either side may be strided): one hamt_gather_rows launch with the
    identity index -- the in-place `cat` / `stack` of the no-grad paths (history cache, vision buffer)."""
    R, W = src2d.shape
    assert dst2d.shape[0] == R and dst2d.stride(1) == 1 and src2d.stride(1) == 1 and col0 + W <= dst2d.shape[1]
    L.check(L.load().hamt_gather_rows(R, W, _p(src2d), _ld(src2d), None, None, W, _p(dst2d), _ld(dst2d), col0, _stream()), "hamt_gather_rows")
    return dst2d


class Add3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c):
        _chk(a, "Add3Fn")
        a, b = a.contiguous(), b.contiguous()
        c = c.contiguous() if c is not None else None
        out = torch.empty_like(a)
        L.check(L.load().hamt_add3(a.numel(), _p(a), _p(b), _p(c), _p(out), _stream()), "hamt_add3")
        ctx.has_c = c is not None
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g, (g if ctx.has_c else None)


def add3(a, b, c=None):
    return Add3Fn.apply(a, b, c)


class MeanMidFn(torch.autograd.Function):
    """(B,S,H) -> (B,H) mean over S (panorama mean pooling, vilmodel.py:563-564)."""

    @staticmethod
    def forward(ctx, x):
        _chk(x, "MeanMidFn")
        x = x.contiguous()
        B, S, H = x.shape
        y = torch.empty(B, H, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_mean_mid_fwd(B, S, H, _p(x), _p(y), _stream()), "hamt_mean_mid_fwd")
        ctx.shape = (B, S, H)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, S, H = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty(B, S, H, dtype=torch.float32, device=dy.device)
        L.check(L.load().hamt_mean_mid_bwd(B, S, H, _p(dy), _p(dx), _stream()), "hamt_mean_mid_bwd")
        return dx


class MulBcastFn(torch.autograd.Function):
    """y[b,s,:] = a[b,s,:] * c[b,:]  (SAP fusion ob*txt_cls pretrain_cmt.py:176; ITM cls product vilmodel.py:722).
    `c` may be a strided row view such as txt_embeds[:, 0]."""

    @staticmethod
    def forward(ctx, a, c):
        _chk(a, "MulBcastFn")
        a = a.contiguous()
        B, S, H = a.shape
        if c.stride(-1) != 1 or (c.stride(0) % 4):
            c = c.contiguous()
        y = torch.empty_like(a)
        L.check(L.load().hamt_mul_bcast_fwd(B, S, H, _p(a), _p(c), c.stride(0), _p(y), _stream()), "hamt_mul_bcast_fwd")
        ctx.save_for_backward(a, c)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, c = ctx.saved_tensors
        B, S, H = a.shape
        dy = dy.contiguous()
        da = torch.empty_like(a)
        dc = torch.empty(B, H, dtype=torch.float32, device=a.device)
        L.check(L.load().hamt_mul_bcast_bwd(B, S, H, _p(a), _p(c), c.stride(0), _p(dy), _p(da), _p(dc), _stream()), "hamt_mul_bcast_bwd")
        return da, dc


class FillWhereZeroFn(torch.autograd.Function):
    """x.masked_fill(flag == 0, value) (pretrain_cmt.py:177 does it in place on a fresh tensor; the result
    is the same object-wise for callers); backward zeroes the gradient at the filled positions."""

    @staticmethod
    def forward(ctx, x, flag, value):
        _chk(x, "FillWhereZeroFn")
        flag = flag.contiguous()
        assert flag.numel() == x.numel()
        y = x.contiguous().clone()
        L.check(L.load().hamt_fill_where_zero(y.numel(), _p(flag), _p(y), float(value), _stream()), "hamt_fill_where_zero")
        ctx.save_for_backward(flag)
        return y

    @staticmethod
    def backward(ctx, g):
        (flag,) = ctx.saved_tensors
        g = g.contiguous().clone()
        L.check(L.load().hamt_fill_where_zero(g.numel(), _p(flag), _p(g), 0.0, _stream()), "hamt_fill_where_zero")
        return g, None, None


class DropoutFn(torch.autograd.Function):
    """Feature dropout (finetune model_HAMT.py:32-52); same counter-based mask replayed in backward."""

    @staticmethod
    def forward(ctx, x, p):
        _chk(x, "DropoutFn")
        x = x.contiguous()
        y = torch.empty_like(x)
        ctx.cid, ctx.p = next_call_id(), float(p)
        L.check(L.load().hamt_dropout(x.numel(), _p(x), _p(y), ctx.p, ctx.cid, _p(rng_state(x.device)), _stream()), "hamt_dropout")
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        dx = torch.empty_like(g)
        L.check(L.load().hamt_dropout(g.numel(), _p(g), _p(dx), ctx.p, ctx.cid, _p(rng_state(g.device)), _stream()), "hamt_dropout")
        return dx, None


def fill_where_zero(x, flag, value):
    return FillWhereZeroFn.apply(x, flag, value)


def mean_mid(x):
    return MeanMidFn.apply(x)


def mul_bcast(a, c):
    return MulBcastFn.apply(a, c)


def embed_sum(ids, word, pos, typ):
    return EmbedSumFn.apply(ids, word, pos, typ)


def dropout(x, p, training):
    if not training or p <= 0:
        return x
    return DropoutFn.apply(x, p)


# ------------------------------------------------------------------------------------------ losses
class CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy(x, label, reduction='none') (pretrain_cmt.py:154, 180, 259)."""

    @staticmethod
    def forward(ctx, x, label):
        _chk(x, "CrossEntropyFn")
        assert x.dim() == 2
        if x.stride(1) != 1:
            x = x.contiguous()
        R, Cc = x.shape
        label = label.contiguous()
        loss = torch.empty(R, dtype=torch.float32, device=x.device)
        lse = torch.empty(R, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_ce_fwd(R, Cc, _p(x), x.stride(0), _p(label), _p(loss), _p(lse), _stream()), "hamt_ce_fwd")
        ctx.save_for_backward(x, label, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, label, lse = ctx.saved_tensors
        R, Cc = x.shape
        g = g.contiguous()
        ld = (Cc + 7) // 8 * 8                       # keep rows 16-byte aligned for the following GEMMs
        buf = torch.empty(R, ld, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_ce_bwd(R, Cc, _p(x), x.stride(0), _p(label), _p(lse), _p(g), _p(buf), ld, _stream()), "hamt_ce_bwd")
        return buf[:, :Cc], None


class MseFn(torch.autograd.Function):
    """F.mse_loss(x, t, reduction='none') (pretrain_cmt.py:197, 219)."""

    @staticmethod
    def forward(ctx, x, t):
        _chk(x, "MseFn")
        x, t = x.contiguous(), t.contiguous().to(torch.float32)
        loss = torch.empty_like(x)
        L.check(L.load().hamt_mse_fwd(x.numel(), _p(x), _p(t), _p(loss), _stream()), "hamt_mse_fwd")
        ctx.save_for_backward(x, t)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        L.check(L.load().hamt_mse_bwd(x.numel(), _p(x), _p(t), _p(g), _p(dx), _stream()), "hamt_mse_bwd")
        return dx, None


class KlFn(torch.autograd.Function):
    """F.kl_div(F.log_softmax(x, -1), t, reduction='none').sum(1) (pretrain_cmt.py:239-240)."""

    @staticmethod
    def forward(ctx, x, t):
        _chk(x, "KlFn")
        assert x.dim() == 2
        if x.stride(1) != 1:
            x = x.contiguous()
        t = t.contiguous().to(torch.float32)
        R, Cc = x.shape
        loss = torch.empty(R, dtype=torch.float32, device=x.device)
        lse = torch.empty(R, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_kl_fwd(R, Cc, _p(x), x.stride(0), _p(t), Cc, _p(loss), _p(lse), _stream()), "hamt_kl_fwd")
        ctx.save_for_backward(x, t, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, t, lse = ctx.saved_tensors
        R, Cc = x.shape
        g = g.contiguous()
        ld = (Cc + 7) // 8 * 8
        buf = torch.empty(R, ld, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_kl_bwd(R, Cc, _p(x), x.stride(0), _p(t), Cc, _p(lse), _p(g), _p(buf), ld, _stream()), "hamt_kl_bwd")
        return buf[:, :Cc], None


def cross_entropy(x, label):
    return CrossEntropyFn.apply(x, label)


def mse_loss(x, t):
    return MseFn.apply(x, t)


class A2cFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, value, ent, reward, mask, last_value, gamma, ent_w):
        T, B = logp.shape
        dev = logp.device
        f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
        logp_, value_, ent_, reward_, mask_, last_ = f(logp), f(value), f(ent), f(reward), f(mask), f(last_value)
        ret = torch.empty(T, B, dtype=torch.float32, device=dev)
        out = torch.empty(B, 3, dtype=torch.float32, device=dev)
        L.check(L.load().hamt_a2c_fwd(T, B, _p(reward_), _p(mask_), _p(value_), _p(logp_), _p(ent_), _p(last_), float(gamma), float(ent_w),
                                      _p(ret), _p(out), _stream()), "hamt_a2c_fwd")
        ctx.save_for_backward(ret, mask_, value_)
        ctx.meta = (T, B, float(ent_w), ent is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        ret, mask_, value_ = ctx.saved_tensors
        T, B, ent_w, has_ent = ctx.meta
        dev = ret.device
        # the caller reduces `out` with ONE scalar weight per rollout (sum, / total, / batch: agent_cmt.py:508-514)
        g = dout.reshape(-1)[:1].to(torch.float32).contiguous()
        dlogp = torch.empty(T, B, dtype=torch.float32, device=dev)
        dvalue = torch.empty(T, B, dtype=torch.float32, device=dev)
        dent = torch.empty(T, B, dtype=torch.float32, device=dev) if has_ent else None
        L.check(L.load().hamt_a2c_bwd(T, B, _p(ret), _p(mask_), _p(value_), ent_w, _p(g), _p(dlogp), _p(dvalue), _p(dent), _stream()), "hamt_a2c_bwd")
        return dlogp, dvalue, dent, None, None, None, None, None


def a2c_loss(logp, value, reward, mask, last_value=None, entropy=None, gamma=0.9, entropy_weight=0.01, normalize="total"):
    """The agent's RL loss over a whole rollout in two launches (finetune_src/r2r/agent_cmt.py:476-518): `logp`, `value`,
    `reward`, `mask` (and `entropy` for feedback == 'sample') are [T, B]; `last_value` [B] is the critic's value of the last
    state for episodes that have not ended and 0 for the others (:480-484).  normalize: 'total' (/ mask.sum()), 'batch'
    (/ B) or 'none' (:508-514).  Returns (loss, {policy, critic, entropy sums}) -- the sums are what the reference logs."""
    out = A2cFn.apply(logp, value, entropy, reward, mask, last_value, gamma, entropy_weight)
    parts = out.sum(0)
    loss = parts.sum()
    if normalize == "total":
        loss = loss / mask.to(torch.float32).sum()
    elif normalize == "batch":
        loss = loss / logp.shape[1]
    else:
        assert normalize == "none", normalize
    return loss, {"policy": parts[0].detach(), "critic": parts[1].detach(), "entropy": parts[2].detach()}


POLICY_MODES = {"teacher": 0, "argmax": 1, "sample": 2}      # HAMT_POLICY_*


def _fp32_rows(logit):
    """a [B, V] logit as the step kernels read it: detached, fp32, unit column stride (no copy when it already is)"""
    x = logit.detach()
    return x if x.dtype == torch.float32 and x.stride(1) == 1 else x.to(torch.float32).contiguous()


def _check_step_args(op_name, dev, specs):
    """every (name, tensor or None, dtype, shape) of `specs`: a contiguous tensor of that dtype and shape on `dev`"""
    for name, t_, dt, shape in specs:
        if t_ is not None and (t_.dtype != dt or tuple(t_.shape) != shape or not t_.is_contiguous() or t_.device != dev):
            raise L.HamtError(f"{op_name}: {name} must be a contiguous {dt} tensor of shape {shape} on {dev}, got {t_.dtype} {tuple(t_.shape)} on {t_.device}")


def _grad_arg(g):
    """a [B] gradient with element stride 1 or 0 (the expanded gradient of a plain sum) goes in as it is: no copy kernel"""
    if g is None:
        return None, 0
    if g.dtype != torch.float32 or g.stride(0) not in (0, 1):
        g = g.to(torch.float32).contiguous()
    return g, g.stride(0)


class PolicyStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, target, bt_mask, cand_len, ended, mask, ob_ang, hist_len, forced_action, uniform, mode, ignoreid, call_id, out):
        _chk(logit, "policy_step")
        x = _fp32_rows(logit)
        B, V = x.shape
        dev = x.device
        A = 0 if ob_ang is None else ob_ang.shape[-1]
        _check_step_args("policy_step", dev, (
            ("target", target, torch.int64, (B,)), ("bt_mask", bt_mask, torch.uint8, (B, V)), ("cand_len", cand_len, torch.int32, (B,)),
            ("ended", ended, torch.uint8, (B,)), ("mask", mask, torch.float32, (B,)), ("ob_ang", ob_ang, torch.float32, (B, V, A)),
            ("hist_len", hist_len, torch.int32, (B,)), ("forced_action", forced_action, torch.int64, (B,)),
            ("uniform", uniform, torch.float32, (B,))))
        ml, logp, ent = out if out is not None else (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
        action = torch.empty(B, dtype=torch.int64, device=dev)
        env_action = torch.empty(B, dtype=torch.int32, device=dev)
        prev_angle = torch.empty(B, A, dtype=torch.float32, device=dev)
        lse = torch.empty(B, 2, dtype=torch.float32, device=dev)
        L.check(L.load().hamt_policy_step_fwd(B, V, A, mode, int(ignoreid), _p(x), x.stride(0), _p(target), _p(bt_mask), _p(cand_len), _p(ended),
                                              _p(ob_ang), _p(forced_action), _p(uniform), _p(rng_state(dev)), int(call_id), _p(ml), _p(action),
                                              _p(logp), _p(ent), _p(mask), _p(env_action), _p(prev_angle) if A else None, _p(hist_len), _p(lse),
                                              _stream()), "hamt_policy_step_fwd")
        ctx.save_for_backward(x, target, bt_mask, action, lse)
        ctx.meta = (mode, int(ignoreid))
        ctx.mark_non_differentiable(action, env_action, prev_angle)
        ctx.set_materialize_grads(False)       # (no zero-filled gradients for the outputs nobody differentiates: three fill kernels per step)
        if mode != POLICY_MODES["sample"]:
            ent = None
        return ml, logp, ent, action, env_action, prev_angle

    @staticmethod
    def backward(ctx, g_ml, g_logp, g_ent, *_):
        x, target, bt_mask, action, lse = ctx.saved_tensors
        mode, ignoreid = ctx.meta
        B, V = x.shape
        (g_ml, s_ml), (g_logp, s_logp), (g_ent, s_ent) = _grad_arg(g_ml), _grad_arg(g_logp), _grad_arg(g_ent)
        dx = torch.empty(B, V, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_policy_step_bwd(B, V, mode, ignoreid, _p(x), x.stride(0), _p(target), _p(bt_mask), _p(action), _p(lse), _p(g_ml),
                                              _p(g_logp), _p(g_ent), s_ml, s_logp, s_ent, _p(dx), V, _stream()), "hamt_policy_step_bwd")
        return (dx,) + (None,) * 13


def policy_step(logit, cand_len, ended, mask, mode="sample", target=None, bt_mask=None, ob_ang=None, hist_len=None, forced_action=None,
                uniform=None, ignoreid=-100, call_id=None, out=None):
    """The decision and loss side of one rollout step of the finetune agents (finetune_src/r2r/agent_cmt.py:336-401) in one launch,
    and one more for its backward: `logit` [B, V <= 256] fp32 (-inf at non-candidates) is the only differentiable input.  `mode` is
    the agent's feedback ('teacher', 'argmax', 'sample'); `target` [B] int64 (`ignoreid` = none), `bt_mask` [B, V] uint8,
    `cand_len` [B] int32, `ob_ang` [B, V, A] fp32; `forced_action` [B] int64 overrides the choice and `uniform` [B] fp32 the draws
    of 'sample' (otherwise a counter hash of ops.rng_state, `call_id` and the row).  `ended` [B] uint8, `mask` [B] fp32 and
    `hist_len` [B] int32 are updated IN PLACE (:447, :418-420, :399-401).  `out` = (ml, logp, ent) [B] fp32 tensors to write into
    (rows of a recorder's [T, B] arrays) instead of fresh ones.  Returns (ml, logp, ent, action, env_action, prev_angle): the
    per-row cross-entropy on the unmasked logits, log pi(a_t), the entropy (None unless 'sample'), a_t int64, the environment's
    action int32 (-1 = stop / ignored / ended) and the chosen candidate's angle feature [B, A].  Nothing in here reads the device
    from the host; a row whose every slot is masked yields env_action -1 and zero gradients (hamt.h)."""
    return PolicyStepFn.apply(logit, target, bt_mask, cand_len, ended, mask, ob_ang, hist_len, forced_action, uniform, POLICY_MODES[mode],
                              ignoreid, next_call_id() if call_id is None else call_id, out)


STOP_LOGITS = {"index": 0, "value": 1}                       # HAMT_STOP_LOGIT_*


class PolicyRefStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, act_logit, obj_logit, obj_len, cand_len, ended, mask, target, ref_target, obj_id, goal_obj, bt_mask, ob_ang, hist_len,
                forced_action, uniform, mode, stop_logit, last_step, ignoreid, call_id, pred_obj, pred_obj_id, out):
        _chk(act_logit, "policy_ref_step")
        if act_logit.dim() != 2 or obj_logit.dim() != 2 or obj_logit.shape[0] != act_logit.shape[0] or obj_logit.device != act_logit.device:
            raise L.HamtError(f"policy_ref_step: act_logit [B, V] and obj_logit [B, O] on one device, got {tuple(act_logit.shape)} on "
                              f"{act_logit.device} and {tuple(obj_logit.shape)} on {obj_logit.device}")
        x, xo = _fp32_rows(act_logit), _fp32_rows(obj_logit)
        (B, V), O = x.shape, xo.shape[1]
        dev = x.device
        A = 0 if ob_ang is None else ob_ang.shape[-1]
        i32_, i64_, u8_, f32_ = torch.int32, torch.int64, torch.uint8, torch.float32
        _check_step_args("policy_ref_step", dev, (
            ("obj_len", obj_len, i32_, (B,)), ("cand_len", cand_len, i32_, (B,)), ("ended", ended, u8_, (B,)), ("mask", mask, f32_, (B,)),
            ("target", target, i64_, (B,)), ("ref_target", ref_target, i64_, (B,)), ("obj_id", obj_id, i32_, (B, O)),
            ("goal_obj", goal_obj, i32_, (B,)), ("bt_mask", bt_mask, u8_, (B, V)), ("ob_ang", ob_ang, f32_, (B, V, A)),
            ("hist_len", hist_len, i32_, (B,)), ("forced_action", forced_action, i64_, (B,)), ("uniform", uniform, f32_, (B,)),
            ("pred_obj", pred_obj, i32_, (B,)), ("pred_obj_id", pred_obj_id, i32_, (B,))))
        if (obj_id is None) != (goal_obj is None) and ref_target is None:
            raise L.HamtError("policy_ref_step: the object target comes from ref_target, or from obj_id AND goal_obj")
        ml, ref, logp, ent = out if out is not None else (torch.empty(B, dtype=f32_, device=dev) for _ in range(4))
        action = torch.empty(B, dtype=i64_, device=dev)
        env_action = torch.empty(B, dtype=i32_, device=dev)
        prev_angle = torch.empty(B, A, dtype=f32_, device=dev)
        lse = torch.empty(B, 3, dtype=f32_, device=dev)
        saved = torch.empty(B, 3, dtype=i32_, device=dev)
        L.check(L.load().hamt_policy_ref_step_fwd(
            B, V, O, A, mode, stop_logit, int(bool(last_step)), int(ignoreid), _p(x), x.stride(0), _p(xo), xo.stride(0), _p(obj_len), _p(cand_len),
            _p(target), _p(ref_target), _p(obj_id), _p(goal_obj), _p(bt_mask), _p(ended), _p(ob_ang), _p(forced_action), _p(uniform),
            _p(rng_state(dev)), int(call_id), _p(ml), _p(ref), _p(action), _p(logp), _p(ent), _p(mask), _p(env_action),
            _p(prev_angle) if A else None, _p(hist_len), _p(pred_obj), _p(pred_obj_id) if obj_id is not None else None, _p(lse), _p(saved),
            _stream()), "hamt_policy_ref_step_fwd")
        ctx.save_for_backward(x, xo, bt_mask, action, lse, saved)
        ctx.meta = (mode, stop_logit)
        ctx.mark_non_differentiable(action, env_action, prev_angle)
        ctx.set_materialize_grads(False)
        if mode != POLICY_MODES["sample"]:
            ent = None
        return ml, ref, logp, ent, action, env_action, prev_angle

    @staticmethod
    def backward(ctx, g_ml, g_ref, g_logp, g_ent, *_):
        x, xo, bt_mask, action, lse, saved = ctx.saved_tensors
        mode, stop_logit = ctx.meta
        (B, V), O = x.shape, xo.shape[1]
        (g_ml, s_ml), (g_ref, s_ref), (g_logp, s_logp), (g_ent, s_ent) = _grad_arg(g_ml), _grad_arg(g_ref), _grad_arg(g_logp), _grad_arg(g_ent)
        dx = torch.empty(B, V, dtype=torch.float32, device=x.device)
        dxo = torch.empty(B, O, dtype=torch.float32, device=x.device)
        L.check(L.load().hamt_policy_ref_step_bwd(B, V, O, mode, stop_logit, _p(x), x.stride(0), _p(xo), xo.stride(0), _p(bt_mask), _p(action),
                                                  _p(lse), _p(saved), _p(g_ml), _p(g_ref), _p(g_logp), _p(g_ent), s_ml, s_ref, s_logp, s_ent,
                                                  _p(dx), V, _p(dxo), O, _stream()), "hamt_policy_ref_step_bwd")
        return (dx, dxo) + (None,) * 21


def policy_ref_step(act_logit, obj_logit, obj_len, cand_len, ended, mask, mode="sample", stop_logit="index", target=None, ref_target=None,
                    obj_id=None, goal_obj=None, bt_mask=None, ob_ang=None, hist_len=None, forced_action=None, uniform=None, last_step=False,
                    ignoreid=-100, call_id=None, pred_obj=None, pred_obj_id=None, out=None):
    """`policy_step` for REVERIE's agent (finetune_src/reverie/agent.py:253-307), one launch and one more for its backward.
    `act_logit` [B, V] (V = ob_img_max_len, V + 1 <= 256) and `obj_logit` [B, O <= 256] are the differentiable inputs; the action row is
    act_logit plus ONE column V that stands for STOP: with stop_logit='index' the best object's INDEX as a float, exactly what the
    reference writes (:253-254; no gradient reaches obj_logit through the action row), with 'value' the best object's logit (its
    gradient goes to the arg-max element; ties: the lowest index).  The imitation cross-entropy is taken on the back-track-MASKED row
    (:269, :274); a `target` >= cand_len - 1 means STOP (the reference's V and nav_observe's cand_len - 1 alike).  The object
    cross-entropy `ref` (:275) reads `ref_target` [B] int64, or derives it from `obj_id` int32 [B, O] and `goal_obj` int32 [B]: the
    goal's first slot where the teacher says STOP, else ignored.  `obj_len` int32 [B] is the TRUE object count (0 allowed).
    env_action is -1 iff a_t >= V, a_t == ignoreid or the episode had ended.  `pred_obj` / `pred_obj_id` int32 [B] are updated IN PLACE
    like `ended`, `mask`, `hist_len`: where (a_t >= V or `last_step`) and the episode had not ended, the arg-max of
    obj_logit[b, :obj_len[b]] and its id, -1 for a viewpoint without objects (:299-304).  `out` = (ml, ref, logp, ent).
    Returns (ml, ref, logp, ent, action, env_action, prev_angle)."""
    return PolicyRefStepFn.apply(act_logit, obj_logit, obj_len, cand_len, ended, mask, target, ref_target, obj_id, goal_obj, bt_mask, ob_ang,
                                 hist_len, forced_action, uniform, POLICY_MODES[mode], STOP_LOGITS[stop_logit], last_step, ignoreid,
                                 next_call_id() if call_id is None else call_id, pred_obj, pred_obj_id, out)


NAV_TEACHER_MODES = {"path_step": 0, "path_index": 1, "shortest": 2}      # HAMT_NAV_*
NAV_EVAL_COLS = ("nav_error", "oracle_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "oracle_success", "DTW", "nDTW",
                 "SDTW", "CLS")
NAV_GOALS_EVAL_COLS = ("trajectory_steps", "trajectory_lengths", "success", "oracle_success", "spl", "gp", "spl_ratio")
NAV_BACK_EVAL_COLS = ("nav_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "DTW", "nDTW", "SDTW", "CLS")


def _nav_arg(name, t_, dt, shape, dev):
    if t_.dtype != dt or tuple(t_.shape) != tuple(shape) or not t_.is_contiguous() or t_.device != dev:
        raise L.HamtError(f"{name} must be a contiguous {dt} tensor of shape {tuple(shape)} on {dev}, got {t_.dtype} {tuple(t_.shape)} on {t_.device}")
    return t_


def nav_observe(ep, t, cand_node, cand_len, ended, mode="path_step", ignoreid=-100, target=True, bt_mask=True):
    """Before the policy step of step `t`, one launch for the B episodes of `ep` (agent.NavEpisodes): the teacher's slot
    (agent_cmt.py::_teacher_action over env.py::_teacher_path_action, `mode` in NAV_TEACHER_MODES) and the back-track mask (:342-349)
    from `cand_node` int32 [B, V] (the local node of each navigable candidate, -1 = padding), `cand_len` int32 [B] (STOP slot counted)
    and `ended` uint8 [B].  Returns (target int64 [B] or None, bt_mask uint8 [B, V] or None); nothing is read from the host."""
    _chk(cand_node, "nav_observe")
    dev, (B, V), g = cand_node.device, cand_node.shape, ep.graphs
    _nav_arg("nav_observe: cand_node", cand_node, torch.int32, (ep.B, V), dev)
    _nav_arg("nav_observe: cand_len", cand_len, torch.int32, (B,), dev)
    _nav_arg("nav_observe: ended", ended, torch.uint8, (B,), dev)
    tgt = torch.empty(B, dtype=torch.int64, device=dev) if target else None
    btm = torch.empty(B, V, dtype=torch.uint8, device=dev) if bt_mask else None
    L.check(L.load().hamt_nav_observe(B, V, NAV_TEACHER_MODES[mode], int(t), int(ignoreid), ep.G_max, ep.path_cap, _p(g.nxt), _p(g.scan_offset),
                                      _p(g.scan_n), _p(ep.scan), _p(cand_node), _p(cand_len), _p(ended), _p(ep.cur), _p(ep.goal), _p(ep.gt),
                                      _p(ep.gt_len), _p(ep.path), _p(ep.path_len), _p(ep.anomalies), _p(tgt), _p(btm), _stream()), "hamt_nav_observe")
    return tgt, btm


def nav_advance(ep, cand_node, env_action, mask, reward):
    """After the policy step, one launch: `env_action` int32 [B] (-1 = stop / ignored / ended) moves the episodes of `ep` IN PLACE
    (current node, path, DTW row, last_dist / last_ndtw), and the shaped reward of the step (agent_cmt.py:407-445; `mask` fp32 [B] =
    1 - ended before the step) is written into `reward` fp32 [B] (row t of a recorder's array)."""
    _chk(cand_node, "nav_advance")
    dev, (B, V), g = cand_node.device, cand_node.shape, ep.graphs
    _nav_arg("nav_advance: cand_node", cand_node, torch.int32, (ep.B, V), dev)
    _nav_arg("nav_advance: env_action", env_action, torch.int32, (B,), dev)
    _nav_arg("nav_advance: mask", mask, torch.float32, (B,), dev)
    _nav_arg("nav_advance: reward", reward, torch.float32, (B,), dev)
    L.check(L.load().hamt_nav_advance(B, V, ep.G_max, ep.path_cap, _p(g.dist), _p(g.scan_offset), _p(g.scan_n), _p(ep.scan), _p(cand_node),
                                      _p(env_action), _p(mask), _p(ep.cur), _p(ep.goal), _p(ep.gt), _p(ep.gt_len), _p(ep.path), _p(ep.path_len),
                                      _p(ep.dtw_row), _p(ep.last_dist), _p(ep.last_ndtw), _p(ep.anomalies), _p(reward), _stream()), "hamt_nav_advance")
    return reward


def nav_eval(graphs, scan, path, path_len, gt, gt_len):
    """env.py::_eval_item for N finished trajectories in one launch: `scan` int32 [N] (index into `graphs`, an agent.NavGraphs on the
    device), `path` int32 [N, P_max] / `gt` int32 [N, G_max] of local node ids with their lengths.  Returns fp64 [N, 11] in the column
    order NAV_EVAL_COLS."""
    _chk(path, "nav_eval")
    dev, (N, P), G = path.device, path.shape, gt.shape[1]
    _nav_arg("nav_eval: scan", scan, torch.int32, (N,), dev)
    _nav_arg("nav_eval: path", path, torch.int32, (N, P), dev)
    _nav_arg("nav_eval: path_len", path_len, torch.int32, (N,), dev)
    _nav_arg("nav_eval: gt", gt, torch.int32, (N, G), dev)
    _nav_arg("nav_eval: gt_len", gt_len, torch.int32, (N,), dev)
    out = torch.empty(N, len(NAV_EVAL_COLS), dtype=torch.float64, device=dev)
    L.check(L.load().hamt_nav_eval(N, P, G, _p(graphs.dist), _p(graphs.scan_offset), _p(graphs.scan_n), _p(scan), _p(path), _p(path_len), _p(gt),
                                   _p(gt_len), _p(out), _stream()), "hamt_nav_eval")
    return out


def nav_advance_goals(ep, cand_node, env_action, mask, reward):
    """`nav_advance` for episodes whose goal is a set of nodes (agent.GoalSetEpisodes: CVDN's end_panos, REVERIE's viewpoints the
    object is visible from): the move, `last_dist` = the fp32 minimum distance over the set (0 for an empty set) and the reward of
    cvdn/agent.py:174-203 = reverie/agent.py:337-366 -- a stop is right only AT a goal, a move earns +1 / -1 / 0 -- into `reward`."""
    _chk(cand_node, "nav_advance_goals")
    dev, (B, V), g = cand_node.device, cand_node.shape, ep.graphs
    _nav_arg("nav_advance_goals: cand_node", cand_node, torch.int32, (ep.B, V), dev)
    _nav_arg("nav_advance_goals: env_action", env_action, torch.int32, (B,), dev)
    _nav_arg("nav_advance_goals: mask", mask, torch.float32, (B,), dev)
    _nav_arg("nav_advance_goals: reward", reward, torch.float32, (B,), dev)
    L.check(L.load().hamt_nav_advance_goals(B, V, ep.E_max, ep.path_cap, _p(g.dist), _p(g.scan_offset), _p(g.scan_n), _p(ep.scan), _p(cand_node),
                                            _p(env_action), _p(mask), _p(ep.cur), _p(ep.goals), _p(ep.goal_len), _p(ep.path), _p(ep.path_len),
                                            _p(ep.last_dist), _p(reward), _stream()), "hamt_nav_advance_goals")
    return reward


def nav_advance_back(ep, cand_node, env_action, mask, reward, ended, end_on_miss=True):
    """`nav_advance` for return trips (agent.ReturnEpisodes, r2r/agent_r2rback.py:192-198 and :227-276), after the policy step has set
    `ended` |= stop: the reward is judged against the mid-stop until the first STOP and against the path's end after it; the first
    STOP records `ep.midstop_at`, sets `ep.first_ended` and takes `ended` back to 0 -- or, with `end_on_miss` (RL training), leaves the
    episode ended when the mid-stop was missed by 3 m or more.  `ended` uint8 [B] is the recorder's, updated IN PLACE."""
    _chk(cand_node, "nav_advance_back")
    dev, (B, V), g = cand_node.device, cand_node.shape, ep.graphs
    _nav_arg("nav_advance_back: cand_node", cand_node, torch.int32, (ep.B, V), dev)
    _nav_arg("nav_advance_back: env_action", env_action, torch.int32, (B,), dev)
    _nav_arg("nav_advance_back: mask", mask, torch.float32, (B,), dev)
    _nav_arg("nav_advance_back: reward", reward, torch.float32, (B,), dev)
    _nav_arg("nav_advance_back: ended", ended, torch.uint8, (B,), dev)
    L.check(L.load().hamt_nav_advance_back(B, V, ep.G_max, ep.path_cap, int(bool(end_on_miss)), _p(g.dist), _p(g.scan_offset), _p(g.scan_n),
                                           _p(ep.scan), _p(cand_node), _p(env_action), _p(mask), _p(ep.cur), _p(ep.goal), _p(ep.midstop), _p(ep.gt),
                                           _p(ep.gt_len), _p(ep.path), _p(ep.path_len), _p(ep.dtw_row), _p(ep.last_dist), _p(ep.last_ndtw),
                                           _p(ep.first_ended), _p(ep.midstop_at), _p(ended), _p(ep.anomalies), _p(reward), _stream()),
            "hamt_nav_advance_back")
    return reward


def nav_eval_goals(graphs, scan, path, path_len, goals, goal_len, gt=None, gt_len=None):
    """cvdn/env.py::_eval_item (no `gt`: gt_lengths is the start's distance to the nearest goal) or reverie/env.py::_eval_item's
    navigation part (`gt` int32 [N, G_max]: gt_lengths is the ground-truth path's length) for N finished trajectories in one launch;
    `goals` int32 [N, E_max <= 256] with `goal_len`.  Returns fp64 [N, 7] in the column order NAV_GOALS_EVAL_COLS."""
    _chk(path, "nav_eval_goals")
    dev, (N, P), E = path.device, path.shape, goals.shape[1]
    _nav_arg("nav_eval_goals: scan", scan, torch.int32, (N,), dev)
    _nav_arg("nav_eval_goals: path", path, torch.int32, (N, P), dev)
    _nav_arg("nav_eval_goals: path_len", path_len, torch.int32, (N,), dev)
    _nav_arg("nav_eval_goals: goals", goals, torch.int32, (N, E), dev)
    _nav_arg("nav_eval_goals: goal_len", goal_len, torch.int32, (N,), dev)
    G = 0
    if gt is not None:
        G = gt.shape[1]
        _nav_arg("nav_eval_goals: gt", gt, torch.int32, (N, G), dev)
        _nav_arg("nav_eval_goals: gt_len", gt_len, torch.int32, (N,), dev)
    out = torch.empty(N, len(NAV_GOALS_EVAL_COLS), dtype=torch.float64, device=dev)
    L.check(L.load().hamt_nav_eval_goals(N, P, E, G, _p(graphs.dist), _p(graphs.scan_offset), _p(graphs.scan_n), _p(scan), _p(path), _p(path_len),
                                         _p(goals), _p(goal_len), _p(gt), _p(gt_len if gt is not None else None), _p(out), _stream()),
            "hamt_nav_eval_goals")
    return out


def nav_eval_back(graphs, scan, path, path_len, gt, gt_len, midstop, gt_midstop):
    """env.py::R2RBackBatch._eval_item for N finished return trips in one launch: `nav_eval`'s inputs plus `midstop` int32 [N] (where the
    agent made its first STOP, -1 = never) and `gt_midstop` int32 [N].  Returns fp64 [N, 9] in the column order NAV_BACK_EVAL_COLS."""
    _chk(path, "nav_eval_back")
    dev, (N, P), G = path.device, path.shape, gt.shape[1]
    _nav_arg("nav_eval_back: scan", scan, torch.int32, (N,), dev)
    _nav_arg("nav_eval_back: path", path, torch.int32, (N, P), dev)
    _nav_arg("nav_eval_back: path_len", path_len, torch.int32, (N,), dev)
    _nav_arg("nav_eval_back: gt", gt, torch.int32, (N, G), dev)
    _nav_arg("nav_eval_back: gt_len", gt_len, torch.int32, (N,), dev)
    _nav_arg("nav_eval_back: midstop", midstop, torch.int32, (N,), dev)
    _nav_arg("nav_eval_back: gt_midstop", gt_midstop, torch.int32, (N,), dev)
    out = torch.empty(N, len(NAV_BACK_EVAL_COLS), dtype=torch.float64, device=dev)
    L.check(L.load().hamt_nav_eval_back(N, P, G, _p(graphs.dist), _p(graphs.scan_offset), _p(graphs.scan_n), _p(scan), _p(path), _p(path_len),
                                        _p(gt), _p(gt_len), _p(midstop), _p(gt_midstop), _p(out), _stream()), "hamt_nav_eval_back")
    return out


OBS_LAYOUTS = {"pano": 0, "cand": 1}                          # HAMT_OBS_*
OBS_MAX_CAND = 64                                             # HAMT_OBS_MAX_CAND
OBS_VIEWS = 36


def obs_gather(store, ep_scan, cur, view, out, anomalies, layout="pano"):
    """The observations of one rollout step, one launch (csrc/obs.hip): for the B episodes standing on node `cur` int32 [B] of scan
    `ep_scan` int32 [B] (an agent.NavEpisodes' tensors) and looking at `view` int32 [B], what env.py::_get_obs and the agent's
    _cand_pano_feature_variable (`layout` 'pano') or _candidate_variable ('cand') and _history_variable build on the host, gathered
    from `store` (an agent.ObsStore: feat, ang36, cand_cnt, cand_point, cand_node, cand_ang, vp_base, scan_n on the device).
    `out` carries the buffers, every element of which is overwritten: ob_img fp32 [B, W, F], ob_ang fp32 [B, W, A], ob_nav int64 [B, W],
    ob_mask uint8 [B, W], ob_len / cand_len int32 [B], cand_nodes / cand_points int32 [B, W], and hist_img [B, F], hist_pano_img
    [B, 36, F], hist_pano_ang [B, 36, A] or None.  An episode outside its scan or its 36 views becomes STOP alone and adds 1 to
    `anomalies` int32 [>= 1].  Nothing is read from the host."""
    _chk(out.ob_img, "obs_gather")
    dev, (B, W, F), A, C = out.ob_img.device, out.ob_img.shape, out.ob_ang.shape[-1], store.cand_point.shape[1]
    NV = store.feat.shape[0]
    for name, t_, dt, shape in (("feat", store.feat, torch.float32, (NV, OBS_VIEWS, F)), ("ang36", store.ang36, torch.float32, (OBS_VIEWS, OBS_VIEWS, A)),
                                ("cand_cnt", store.cand_cnt, torch.int32, (NV,)), ("cand_point", store.cand_point, torch.int32, (NV, C)),
                                ("cand_node", store.cand_node, torch.int32, (NV, C)), ("cand_ang", store.cand_ang, torch.float32, (NV, C, 12, A)),
                                ("vp_base", store.vp_base, torch.int64, store.scan_n.shape), ("scan_n", store.scan_n, torch.int32, store.scan_n.shape),
                                ("ep_scan", ep_scan, torch.int32, (B,)), ("cur", cur, torch.int32, (B,)), ("view", view, torch.int32, (B,)),
                                ("ob_img", out.ob_img, torch.float32, (B, W, F)), ("ob_ang", out.ob_ang, torch.float32, (B, W, A)),
                                ("ob_nav", out.ob_nav, torch.int64, (B, W)), ("ob_mask", out.ob_mask, torch.uint8, (B, W)),
                                ("ob_len", out.ob_len, torch.int32, (B,)), ("cand_len", out.cand_len, torch.int32, (B,)),
                                ("cand_nodes", out.cand_nodes, torch.int32, (B, W)), ("cand_points", out.cand_points, torch.int32, (B, W)),
                                ("hist_img", out.hist_img, torch.float32, (B, F)), ("hist_pano_img", out.hist_pano_img, torch.float32, (B, OBS_VIEWS, F)),
                                ("hist_pano_ang", out.hist_pano_ang, torch.float32, (B, OBS_VIEWS, A))):
        if t_ is not None:
            _nav_arg("obs_gather: " + name, t_, dt, shape, dev)
    if anomalies.dtype != torch.int32 or anomalies.device != dev or anomalies.numel() < 1:
        raise L.HamtError("obs_gather: anomalies must be an int32 tensor on the outputs' device")
    L.check(L.load().hamt_obs_gather(B, W, F, A, C, OBS_LAYOUTS[layout], _p(store.feat), _p(store.ang36), _p(store.cand_cnt), _p(store.cand_point),
                                     _p(store.cand_node), _p(store.cand_ang), _p(store.vp_base), _p(store.scan_n), _p(ep_scan), _p(cur), _p(view),
                                     _p(out.ob_img), _p(out.ob_ang), _p(out.ob_nav), _p(out.ob_mask), _p(out.ob_len), _p(out.cand_len),
                                     _p(out.cand_nodes), _p(out.cand_points), _p(out.hist_img), _p(out.hist_pano_img), _p(out.hist_pano_ang),
                                     _p(anomalies), _stream()), "hamt_obs_gather")
    return out


def obs_turn(cand_points, env_action, view, view_log_row=None):
    """After the policy step, one launch: `view` int32 [B] becomes the chosen candidate's view index, `cand_points[b, env_action[b]]`
    (what `obs_gather` wrote; make_equiv_action, agent_cmt.py:213-246), where `env_action` int32 [B] is >= 0; a stop (-1) leaves it.
    `view_log_row` int32 [B] receives the resulting views."""
    _chk(cand_points, "obs_turn")
    dev, (B, W) = cand_points.device, cand_points.shape
    _nav_arg("obs_turn: cand_points", cand_points, torch.int32, (B, W), dev)
    _nav_arg("obs_turn: env_action", env_action, torch.int32, (B,), dev)
    _nav_arg("obs_turn: view", view, torch.int32, (B,), dev)
    if view_log_row is not None:
        _nav_arg("obs_turn: view_log_row", view_log_row, torch.int32, (B,), dev)
    L.check(L.load().hamt_obs_turn(B, W, _p(cand_points), _p(env_action), _p(view), _p(view_log_row), _stream()), "hamt_obs_turn")
    return view


OBJ_MAX_WIDTH = 256                                           # HAMT_OBJ_MAX_WIDTH (policy_ref_step's limit on O)


def obj_gather(store, ep_scan, cur, view, out, anomalies):
    """REVERIE's candidate objects of one rollout step, one launch (csrc/obs.hip): for the B episodes standing on node `cur` int32 [B]
    of scan `ep_scan` int32 [B] and looking at `view` int32 [B], what reverie/env.py::_get_obs (:181-215) and the agent's
    _object_variable (reverie/agent.py:125-139) build on the host, gathered from `store` (an agent.ObjStore: obj_off, obj_feat, obj_view,
    obj_pos, obj_id, and its viewpoint store's ang36, vp_base, scan_n, on the device).  `out` carries the buffers, every element of which
    is overwritten: obj_feats fp32 [B, Ow, Fo], obj_angles fp32 [B, Ow, A], obj_poses fp32 [B, Ow, 5], obj_masks uint8 [B, Ow] (one live
    slot at a viewpoint without objects), obj_lens int32 [B] (the true count), obj_ids int32 [B, Ow] (-1 = padding).  An episode
    outside its scan or its 36 views gets one live zero slot, count 0, and adds 1 to `anomalies` int32 [>= 1].  Nothing is read from
    the host."""
    _chk(out.obj_feats, "obj_gather")
    dev, (B, Ow, Fo), A = out.obj_feats.device, out.obj_feats.shape, out.obj_angles.shape[-1]
    NV, NObj, S = store.obj_off.shape[0] - 1, store.obj_feat.shape[0], store.scan_n.shape[0]
    if Ow > OBJ_MAX_WIDTH:
        raise L.HamtError(f"obj_gather: {Ow} object slots, above the supported {OBJ_MAX_WIDTH}")
    for name, t_, dt, shape in (("obj_off", store.obj_off, torch.int64, (NV + 1,)), ("obj_feat", store.obj_feat, torch.float32, (NObj, Fo)),
                                ("obj_view", store.obj_view, torch.int32, (NObj,)), ("obj_pos", store.obj_pos, torch.float32, (NObj, 5)),
                                ("obj_id", store.obj_id, torch.int32, (NObj,)), ("ang36", store.ang36, torch.float32, (OBS_VIEWS, OBS_VIEWS, A)),
                                ("vp_base", store.vp_base, torch.int64, (S,)), ("scan_n", store.scan_n, torch.int32, (S,)),
                                ("ep_scan", ep_scan, torch.int32, (B,)), ("cur", cur, torch.int32, (B,)), ("view", view, torch.int32, (B,)),
                                ("obj_feats", out.obj_feats, torch.float32, (B, Ow, Fo)), ("obj_angles", out.obj_angles, torch.float32, (B, Ow, A)),
                                ("obj_poses", out.obj_poses, torch.float32, (B, Ow, 5)), ("obj_masks", out.obj_masks, torch.uint8, (B, Ow)),
                                ("obj_lens", out.obj_lens, torch.int32, (B,)), ("obj_ids", out.obj_ids, torch.int32, (B, Ow))):
        _nav_arg("obj_gather: " + name, t_, dt, shape, dev)
    if anomalies.dtype != torch.int32 or anomalies.device != dev or anomalies.numel() < 1:
        raise L.HamtError("obj_gather: anomalies must be an int32 tensor on the outputs' device")
    L.check(L.load().hamt_obj_gather(B, Ow, Fo, A, S, NV, NObj, _p(store.obj_off), _p(store.obj_feat), _p(store.obj_view), _p(store.obj_pos),
                                     _p(store.obj_id), _p(store.ang36), _p(store.vp_base), _p(store.scan_n), _p(ep_scan), _p(cur), _p(view),
                                     _p(out.obj_feats), _p(out.obj_angles), _p(out.obj_poses), _p(out.obj_masks), _p(out.obj_lens),
                                     _p(out.obj_ids), _p(anomalies), _stream()), "hamt_obj_gather")
    return out


PRETRAIN_LAYOUTS = {"views36": 0, "cands_first": 1}            # HAMT_PRETRAIN_VIEWS36 / _CANDS_FIRST
PRETRAIN_RECORD, PRETRAIN_MAX_HIST = 8, 32                     # HAMT_PRETRAIN_RECORD / _MAX_HIST
PRETRAIN_OUTPUTS = ("hist_img_fts", "hist_ang_fts", "hist_pano_img_fts", "hist_pano_ang_fts", "hist_img_probs", "hist_mrc_masks", "hist_masks",
                    "hist_lens", "ob_img_fts", "ob_ang_fts", "ob_nav_types", "ob_masks", "ob_lens", "ob_action_viewindex", "ob_action_angles",
                    "ob_progress", "sp_anchor_idxs", "sp_targets")                   # hamt_pretrain_gather's outputs, in its order


def pretrain_gather(store, records, out, Hmax, Omax, layout=0):
    """One pretraining batch, one launch (csrc/pretrain_gather.hip): for the B samples of `records` int32 [B, 8] (data/device_tasks.py),
    what MultiStepNavData.get_input, the task datasets and their collate functions build on the host, gathered from `store` (a
    data.device_store.PretrainStore).  `out`: {name: tensor} over PRETRAIN_OUTPUTS, a missing or None entry = an output the task does not
    have; shapes as the collated batch has them (hist_* [B, Hmax, ...], hist_masks [B, Hmax + 1], ob_* [B, Omax, ...], masks bool, lengths
    and indices int64), every element of which is overwritten.  A record pointing outside the tables gives a sample of zeros and adds 1
    to `store.anomalies`.  Nothing is read from the host."""
    _chk(records, "pretrain_gather")
    dev, B, F, A, P = records.device, records.shape[0], store.F, store.A, store.P
    _nav_arg("pretrain_gather: records", records, torch.int32, (B, PRETRAIN_RECORD), dev)
    if store.device != dev:
        raise L.HamtError(f"pretrain_gather: the store is on {store.device}, the records on {dev}")
    Hmax, Omax, layout = int(Hmax), int(Omax), PRETRAIN_LAYOUTS.get(layout, layout)
    if not 0 <= Hmax <= PRETRAIN_MAX_HIST or Omax < 0 or layout not in (0, 1):
        raise L.HamtError(f"pretrain_gather: Hmax {Hmax} outside [0, {PRETRAIN_MAX_HIST}], Omax {Omax} < 0 or layout {layout} unknown")
    shapes = {"hist_img_fts": (torch.float32, (B, Hmax, F)), "hist_ang_fts": (torch.float32, (B, Hmax, A)),
              "hist_pano_img_fts": (torch.float32, (B, Hmax, OBS_VIEWS, F)), "hist_pano_ang_fts": (torch.float32, (B, Hmax, OBS_VIEWS, A)),
              "hist_img_probs": (torch.float32, (B, Hmax, P)), "hist_mrc_masks": (torch.bool, (B, Hmax)), "hist_masks": (torch.bool, (B, Hmax + 1)),
              "hist_lens": (torch.int64, (B,)), "ob_img_fts": (torch.float32, (B, Omax, F)), "ob_ang_fts": (torch.float32, (B, Omax, A)),
              "ob_nav_types": (torch.int64, (B, Omax)), "ob_masks": (torch.bool, (B, Omax)), "ob_lens": (torch.int64, (B,)),
              "ob_action_viewindex": (torch.int64, (B,)), "ob_action_angles": (torch.float32, (B, 2)), "ob_progress": (torch.float32, (B,)),
              "sp_anchor_idxs": (torch.int64, (B,)), "sp_targets": (torch.float32, (B, OBS_VIEWS, 2))}
    unknown = set(out) - set(shapes)
    if unknown:
        raise L.HamtError(f"pretrain_gather: unknown outputs {sorted(unknown)}")
    ptrs = []
    for name in PRETRAIN_OUTPUTS:
        t_ = out.get(name)
        if t_ is not None:
            _nav_arg("pretrain_gather: " + name, t_, shapes[name][0], shapes[name][1], dev)
        ptrs.append(_p(t_))
    if out.get("hist_img_probs") is not None and store.prob is None:
        raise L.HamtError("pretrain_gather: hist_img_probs asked of a store built without the soft labels (with_probs=False)")
    L.check(L.load().hamt_pretrain_gather(B, Hmax, Omax, F, A, P, store.C, layout, store.NV, store.NS, _p(store.feat), _p(store.prob),
                                          _p(store.ang36), _p(store.cand_cnt), _p(store.cand_view), _p(store.cand_ang), _p(store.step_idx),
                                          _p(store.step_val), _p(store.sp_targets), _p(records), *ptrs, _p(store.anomalies), _stream()),
            "hamt_pretrain_gather")
    return out


def kl_div_logsoftmax(x, t):
    return KlFn.apply(x, t)


# ------------------------------------------------------------------------------------------ validation accumulators
EVAL_SLOTS = 4              # double sums[4], int64 counts[4] (include/hamt.h: hamt_eval_*)


class EvalAccumulator:
    """The device totals of one validation pass: `sums` fp64 [4] and `counts` int64 [4] behind one 64-byte buffer, which eval_ce /
    eval_kl / eval_mse_cols ADD into.  Nothing is read back until `read()`, the pass's one device-to-host copy."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HamtError(f"EvalAccumulator: device is {self.device}; the HAMT kernels run on the GPU only (no CPU fallback)")
        self.buf = torch.zeros(2 * EVAL_SLOTS, dtype=torch.int64, device=self.device)
        self.device = self.buf.device       # ("cuda" -> the current device, with its index)
        self.sums = self.buf[:EVAL_SLOTS].view(torch.float64)
        self.counts = self.buf[EVAL_SLOTS:]
        self._ws = None

    def zero_(self):
        self.buf.zero_()
        return self

    def workspace(self, R: int) -> torch.Tensor:
        """2 R floats of scratch for the row kernels, grown geometrically and kept (every call rewrites what it reads)"""
        if self._ws is None or self._ws.numel() < 2 * R:
            self._ws = torch.empty(max(2 * R, 1024, 0 if self._ws is None else 2 * self._ws.numel()), dtype=torch.float32, device=self.device)
        return self._ws

    def read(self):
        """(sums, counts) as lists of Python floats / ints: ONE device-to-host copy, which waits for the updates in front of it"""
        host = self.buf.cpu()
        return host[:EVAL_SLOTS].view(torch.float64).tolist(), host[EVAL_SLOTS:].tolist()


def _eval_rows(op_name, x, name, dev, dtype=torch.float32):
    """a [R, C] operand of the eval kernels: `dtype`, on `dev`, unit stride in the last dimension; its row stride goes in as ld"""
    if x.dim() == 2 and x.dtype == dtype and x.device == dev and x.numel() == 0:        # (no rows: nothing is read, strides mean nothing)
        return max(1, x.shape[1])
    if x.dim() != 2 or x.dtype != dtype or x.device != dev or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise L.HamtError(f"{op_name}: {name} must be a 2-D {dtype} tensor on {dev} with a contiguous last dimension, got {x.dtype} "
                          f"{tuple(x.shape)} strides {tuple(x.stride())} on {x.device}")
    return _ld(x)


def _eval_acc(op_name, acc, dev):
    if not isinstance(acc, EvalAccumulator) or acc.device != dev:
        raise L.HamtError(f"{op_name}: acc must be an ops.EvalAccumulator on {dev}")


@torch.no_grad()
def eval_ce(x, label, acc):
    """acc.sums[0] += F.cross_entropy(x, label, reduction='sum') over the rows with label >= 0, acc.counts[0] += the rows among them whose
    arg-max (lowest index on ties) is the label, acc.counts[1] += their number -- what validate_mlm / _sap / _itm keep per batch
    (main_r2r.py:355-358).  x fp32 [R, C] with any row stride, label int64 [R].  Two launches, nothing read from the host."""
    _chk(x, "eval_ce")
    dev = x.device
    ldx = _eval_rows("eval_ce", x, "x", dev)
    R, Cc = x.shape
    _check_step_args("eval_ce", dev, [("label", label, torch.int64, (R,))])
    _eval_acc("eval_ce", acc, dev)
    if R == 0 or Cc == 0:
        return acc
    L.check(L.load().hamt_eval_ce(R, Cc, _p(x), ldx, _p(label), _p(acc.workspace(R)), _p(acc.sums), _p(acc.counts), _stream()), "hamt_eval_ce")
    return acc


@torch.no_grad()
def eval_kl(x, t, acc):
    """acc.sums[0] += F.kl_div(log_softmax(x), t, reduction='sum'), acc.counts[0] += rows where argmax x == argmax t,
    acc.counts[1] += R (validate_mrc, main_r2r.py:468-473).  x, t fp32 [R, C] with any row strides."""
    _chk(x, "eval_kl")
    dev = x.device
    ldx = _eval_rows("eval_kl", x, "x", dev)
    ldt = _eval_rows("eval_kl", t, "t", dev)
    R, Cc = x.shape
    if tuple(t.shape) != (R, Cc):
        raise L.HamtError(f"eval_kl: t must have x's shape {(R, Cc)}, got {tuple(t.shape)}")
    _eval_acc("eval_kl", acc, dev)
    if R == 0 or Cc == 0:
        return acc
    L.check(L.load().hamt_eval_kl(R, Cc, _p(x), ldx, _p(t), ldt, _p(acc.workspace(R)), _p(acc.sums), _p(acc.counts), _stream()), "hamt_eval_kl")
    return acc


@torch.no_grad()
def eval_mse_cols(x, t, acc):
    """acc.sums[c] += F.mse_loss(x[:, c], t[:, c], reduction='sum') for the C <= 4 columns of x, t fp32 [R, C] (validate_sar /
    validate_sprel, main_r2r.py:407-409, 437-438).  One launch."""
    _chk(x, "eval_mse_cols")
    dev = x.device
    ldx = _eval_rows("eval_mse_cols", x, "x", dev)
    ldt = _eval_rows("eval_mse_cols", t, "t", dev)
    R, Cc = x.shape
    if tuple(t.shape) != (R, Cc) or not 1 <= Cc <= EVAL_SLOTS:
        raise L.HamtError(f"eval_mse_cols: x and t must share a shape [R, 1 <= C <= {EVAL_SLOTS}], got {tuple(x.shape)} and {tuple(t.shape)}")
    _eval_acc("eval_mse_cols", acc, dev)
    if R == 0:
        return acc
    L.check(L.load().hamt_eval_mse_cols(R, Cc, _p(x), ldx, _p(t), ldt, _p(acc.sums), _stream()), "hamt_eval_mse_cols")
    return acc


# ------------------------------------------------------------------------------------------ range watch on a dense output
RANGE_REC = 4               # int64 rec[4]: at the limit, non-finite, float32 bits of the largest finite |x|, calls (include/hamt.h: hamt_range_audit)


@torch.no_grad()
def range_audit(t, rec):
    """Fold the 2-D fp16 / bf16 / fp32 tensor `t` (unit inner stride, any row stride) into the device record `rec` (int64 [4], contiguous):
    rec[0] += elements with |x| == 65504 (half only: what the clamped store turns an overflow into), rec[1] += non-finite elements,
    rec[2] = max(rec[2], float32 bits of the largest finite |x|), rec[3] += 1.  One launch on the current stream, nothing read back."""
    _chk(t, "range_audit")
    dev = t.device
    if t.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise L.HamtError(f"range_audit: t must be fp16, bf16 or fp32, got {t.dtype}")
    ld = _eval_rows("range_audit", t, "t", dev, t.dtype)
    if not torch.is_tensor(rec) or rec.dtype != torch.int64 or rec.device != dev or tuple(rec.shape) != (RANGE_REC,) or not rec.is_contiguous():
        raise L.HamtError(f"range_audit: rec must be a contiguous int64 [{RANGE_REC}] tensor on {dev}")
    M, N = t.shape
    if N == 0:
        raise L.HamtError("range_audit: t has no columns")
    # (a tensor without rows has no data pointer; the call still counts, and reads nothing through the stand-in)
    L.check(L.load().hamt_range_audit(_p(t) if M > 0 else _p(rec), _dt(t), M, N, ld, _p(rec), _stream()), "hamt_range_audit")
    return rec
