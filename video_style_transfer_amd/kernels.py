"""Tensor-level wrappers over the C ABI (libvst_hip.so).

Every function takes device tensors (bf16 activations/weights, fp32 bias/norm params), checks
shapes, and launches on torch's current HIP stream.  Activations are token-major 2-D views
[rows, C] (row stride may exceed C, e.g. a column slice of a fused QKV buffer).
No CPU fallback exists: a CPU tensor or a missing library raises.

Every pointer handed to the library has either passed one of the validators below (_view, _block, _vec, _table,
_qkv) or was allocated by the wrapper itself a few lines above the call (DESIGN.md "Entry points").
"""
from __future__ import annotations

import torch

from . import _lib

BF16 = torch.bfloat16
F32 = torch.float32
I32 = torch.int32


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- launch profiler (bench.py roofline): HIP events around every launch of an instrumented op
_PROF = None  # list of (kind, symbol, flops, bytes, ev_start, ev_end) while active


def profile_launches(active: bool):
    global _PROF
    _PROF = [] if active else None


def collect_launches():
    """[(kind, kernel symbol or None, flops, bytes, ms, shape)] for the launches recorded since
    profile_launches(True)."""
    torch.cuda.synchronize()
    out = [(k, y, f, b, s.elapsed_time(e), sh) for k, y, f, b, s, e, sh in (_PROF or [])]
    return out


class _Rec:
    __slots__ = ("kind", "flops", "nbytes", "s", "sym", "shape")

    def __init__(self, kind, flops, nbytes, sym=None, shape=None):
        self.kind, self.flops, self.nbytes = kind, flops, nbytes
        self.s = None
        self.sym = sym  # callable -> kernel symbol (evaluated only while profiling)
        self.shape = shape

    def __enter__(self):
        if _PROF is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if a and a[0] is not None:
            return  # the library refused the call (VstError): nothing was launched, nothing is recorded
        if _PROF is not None and self.s is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _PROF.append((self.kind, self.sym() if self.sym else None, self.flops, self.nbytes, self.s, e,
                          self.shape))


GEMM_POLICY = {"tile": 0, "splits": 0}  # 0 = library heuristic (tuning / tests may force)
_ROW_INVARIANT = [0]


class row_invariant:
    """Inside: GEMMs and convs run without split-K (splits = 1 unless GEMM_POLICY forces a count), so every output
    row's bits depend on that row's inputs only, never on how many rows the launch has.  The denoise forward runs
    under it (UNetMotionModel.forward_tokens): a frame-sharded rank then computes exactly the unsharded forward's
    bits for its frames.  (Split-K only ever applied to grids under half a wave of tiles; the forward's token GEMMs
    at the step's shapes never split anyway.)"""

    def __enter__(self):
        _ROW_INVARIANT[0] += 1
        return self

    def __exit__(self, *a):
        _ROW_INVARIANT[0] -= 1


_FUSION_WORLD = [1]


class fusion_world:
    """Inside: the one shape-dependent fusion decision is taken as a P-way frame-sharded rank takes it, so a forward
    here computes exactly the bits of a P-way sharded forward.  The motion attention fused into its q/k/v GEMM
    (vst_gemm_temporal_attention) needs a multiple of 16 pixels, and a rank of the all-to-all exchange holds H*W/P of
    them, so an unsharded forward (or an all-gather rank, which holds all H*W) under fusion_world(P) fuses a layer only
    when (H*W) % (16 P) == 0.  UNetMotionModel.forward_tokens enters it with the shard's world size (or its
    `fusion_world` argument); the all-to-all branch of MotionModule, whose pixels are already split, re-enters it
    with 1."""

    def __init__(self, world: int):
        if world < 1:
            raise ValueError(f"fusion_world({world})")
        self.world = int(world)

    def __enter__(self):
        self._prev = _FUSION_WORLD[0]
        _FUSION_WORLD[0] = self.world
        return self

    def __exit__(self, *a):
        _FUSION_WORLD[0] = self._prev


def fusion_pixel_div() -> int:
    """The P of the enclosing fusion_world (1 outside any)."""
    return _FUSION_WORLD[0]


def _splits():
    s = GEMM_POLICY["splits"]
    return s if s or not _ROW_INVARIANT[0] else 1


_WS = {}
_WS_BYTES = 80 << 20  # fp32 split-K slabs


def gemm_kernel_name(M, N, K, kind):
    """Kernel the library launches for a GEMM / conv of this size (kind: 0 linear, 1 GEGLU, 2 conv,
    3 scalar-gather conv) under the current GEMM_POLICY."""
    name = _lib.load().vst_gemm_kernel_name(M, N, K, kind, GEMM_POLICY["tile"], _splits(), _WS_BYTES)
    return name.decode() if name else None


def _workspace(device):
    """GEMM workspace per (device, stream) (allocated once, reused stream-ordered): the fp32 split-K slabs.  One per
    stream, so GEMMs queued on two streams never share slabs."""
    key = (device, _stream())
    ws = _WS.get(key)
    if ws is None:
        ws = torch.zeros(_WS_BYTES // 4, dtype=F32, device=device)
        _WS[key] = ws
    return ws


# ---- operand validators: what a kernel addresses through a raw pointer is checked here, on the host, first ----
def _fail(fn, name, why):
    raise _lib.VstError(f"{fn}: {name} {why}")


def _on_device(t, dtype, name, fn):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        _fail(fn, name, "must be a device tensor; the HIP path has no CPU fallback")
    if t.dtype != dtype:
        _fail(fn, name, f"expected {dtype}, got {t.dtype}")
    return t


def _view(t, dtype, name, fn, shape=None, rows=None, min_cols=None):
    """A 2-D row view (an operand whose ABI carries a row stride): on the device, `dtype`, unit column stride; with
    `shape` exactly that shape, with `rows` that many rows, with `min_cols` at least that many columns.  A kernel
    given anything else reads or writes outside the view."""
    _on_device(t, dtype, name, fn)
    if t.dim() != 2 or t.stride(1) != 1:
        _fail(fn, name, f"expected a 2-D row-major view, got shape {tuple(t.shape)} stride {t.stride()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        _fail(fn, name, f"shape {tuple(t.shape)} != {tuple(shape)}")
    if (rows is not None and t.shape[0] != rows) or (min_cols is not None and t.shape[1] < min_cols):
        _fail(fn, name, f"shape {tuple(t.shape)}: expected {'any' if rows is None else rows} rows of >= "
                        f"{min_cols or 0} columns")
    return t


def _block(t, dtype, name, fn, shape=None, numel=None):
    """A tensor the kernel addresses as one contiguous block (no row stride in its ABI): on the device, `dtype`,
    contiguous, of `shape` (or of `numel` elements in any shape; neither: any size)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        _fail(fn, name, "must be a device tensor; the HIP path has no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)) \
            or (numel is not None and t.numel() != numel):
        want = f" {tuple(shape)}" if shape is not None else ("" if numel is None else f" [{numel}]")
        _fail(fn, name, f"must be contiguous {dtype}{want}, got {t.dtype} {tuple(t.shape)} stride {t.stride()}")
    return t


def _vec(t, n, name, fn):
    """An fp32 per-channel vector of n elements on the device (bias, gamma, beta), read as float4s."""
    return _block(t, F32, name, fn, numel=n)


def _table(t, rows, cols, name, fn, exact=True, align=True):
    """An fp32 table the kernel reads by row (row_bias, gate, pos, pe): a 2-D device view with unit column stride, at
    least `rows` rows and exactly (exact=False: at least) `cols` columns; align: the rows are read as float4s, so the
    base is 16-byte aligned and the row stride a multiple of 4.  Returns the row stride to pass (a single row's own
    stride is never used: `cols`)."""
    _on_device(t, F32, name, fn)
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < rows or (t.shape[1] != cols if exact else t.shape[1] < cols):
        _fail(fn, name, f"must be a 2-D fp32 view of >= {rows} rows x {cols} columns with unit column stride, got "
                        f"shape {tuple(t.shape)} stride {t.stride()}")
    ld = t.stride(0) if t.shape[0] > 1 else cols
    if align and (ld < cols or ld % 4 or t.data_ptr() % 16):
        _fail(fn, name, f"needs a row stride >= {cols} that is a multiple of 4 and a 16-byte aligned base, got "
                        f"stride {t.stride()}")
    return ld


def _qkv(fn, q, k, v, rows, kv_rows=None, q_shares=False, **like_q):
    """The q/k/v triple of an attention entry: bf16 views of `rows` (k / v: `kv_rows`, default `rows`) rows; k and v
    share one row stride (q_shares: q too, the entries with a single ldqkv); like_q: further views of q's row count
    (o, dout)."""
    kv_rows = rows if kv_rows is None else kv_rows
    for name, t, n in (("q", q, rows), ("k", k, kv_rows), ("v", v, kv_rows)) + tuple((m, t, rows)
                                                                                     for m, t in like_q.items()):
        _view(t, BF16, name, fn, rows=n)
    if k.stride(0) != v.stride(0) or (q_shares and q.stride(0) != k.stride(0)):
        _fail(fn, "q/k/v" if q_shares else "k and v", "must share a row stride")


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _new(out, shape, like, name, fn, dtype=BF16):
    """The output view: `out` validated as exactly `shape`, or a fresh tensor next to `like`."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    return _view(out, dtype, name, fn, shape=shape)


def linear(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, *, x2: torch.Tensor | None = None,
           residual: torch.Tensor | None = None, row_bias: torch.Tensor | None = None, row_bias_div: int = 1,
           out: torch.Tensor | None = None, geglu: bool = False, alg_k2: int | None = None,
           kind: str | None = None, alg_n: int | None = None, act: str | None = None) -> torch.Tensor:
    """out[M, N'] = epilogue([x | x2] @ w^T + bias + row_bias[m // div] + residual); N' = N or N/2 (GEGLU).
    act="gelu": GELU(erf) of (x @ w^T + bias) — no residual / row bias with it."""
    fn = "linear"
    _view(x, BF16, "x", fn)
    _view(w, BF16, "w", fn)
    M, K1 = x.shape
    N, K = w.shape
    if x2 is not None:
        _view(x2, BF16, "x2", fn, rows=M)
        if K1 + x2.shape[1] != K:
            raise _lib.VstError(f"linear: x {tuple(x.shape)} + x2 {tuple(x2.shape)} vs w {tuple(w.shape)}")
    elif K1 != K:
        raise _lib.VstError(f"linear: x {tuple(x.shape)} vs w {tuple(w.shape)}")
    if act not in (None, "gelu") or (act and (geglu or residual is not None or row_bias is not None)):
        raise _lib.VstError(f"linear: act={act!r} supports only bias (no GEGLU / residual / row bias)")
    n_out = N // 2 if geglu else N
    out = _new(out, (M, n_out), x, "out", fn)
    if bias is not None:
        _vec(bias, N, "bias", fn)
    if residual is not None:
        _view(residual, BF16, "residual", fn, shape=(M, n_out))
    ldrb = 0
    if row_bias is not None:
        if row_bias_div <= 0:
            raise _lib.VstError(f"linear: row_bias_div {row_bias_div}")
        rb = row_bias  # (a contiguous table of any rank whose last dimension is N is its [rows, N] form)
        if isinstance(rb, torch.Tensor) and rb.dim() != 2 and rb.is_contiguous() and rb.numel() and rb.shape[-1] == N:
            rb = rb.view(-1, N)
        ldrb = _table(rb, (M - 1) // row_bias_div + 1, N, "row_bias", fn)
    # algorithmic work: the LoRA columns count only their real rank (alg_k2), not the zero padding
    k_alg = K1 + (0 if x2 is None else (x2.shape[1] if alg_k2 is None else alg_k2))
    kind = kind or ("gemm_geglu" if geglu else ("gemm_lora" if x2 is not None and alg_k2 is not None else "gemm"))
    n_alg = N if alg_n is None else alg_n
    with _Rec(kind, 2.0 * M * n_alg * k_alg, 2.0 * (M * k_alg + N * k_alg + M * n_out * (2 if residual is not None else 1)),
              lambda: gemm_kernel_name(M, N, K, 1 if geglu else 0), (M, N, K)):
        ws = _workspace(x.device)
        _lib.call("vst_gemm_ex", _p(x), _ld(x), _p(x2), 0 if x2 is None else _ld(x2), K1, _p(w), _ld(w), M, N, K,
                  _p(bias), _p(row_bias), row_bias_div, ldrb, _p(residual),
                  0 if residual is None else _ld(residual), _p(out), _ld(out), 1 if geglu else (2 if act else 0),
                  GEMM_POLICY["tile"], _splits(), _p(ws), _WS_BYTES, _stream())
    return out


def linear_tn(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[N, K] (bf16) = a^T b with a [M, N] and b [M, K] row-major over the M tokens (vst_gemm_tn): the weight
    gradients of the training backward (dW = g^T x, dA = s v^T x, dB = s g^T u) without transposed copies."""
    fn = "linear_tn"
    _view(a, BF16, "a", fn)
    M, N = a.shape
    _view(b, BF16, "b", fn, rows=M)
    K = b.shape[1]
    out = _new(out, (N, K), a, "out", fn)
    wsb = int(_lib.load().vst_gemm_tn_workspace_bytes(M, N, K))
    ws = torch.empty(max(wsb // 4, 1), dtype=F32, device=a.device) if wsb else None
    with _Rec("gemm_tn", 2.0 * M * N * K, 2.0 * (M * N + M * K + N * K), lambda: "gemm_tn", (N, K, M)):
        _lib.call("vst_gemm_tn", _p(a), _ld(a), _p(b), _ld(b), M, N, K, _p(out), _ld(out), _p(ws), wsb, _stream())
    return out


_LORA_BN = {}
_XATTN_OK = {}


class _Toggle:
    """Context manager around one of the library's process-wide test / A-B switches: `entry(value)` on entry (it
    returns the previous setting), `entry(previous)` on exit; `caches` (host policy answers that depend on the switch)
    are cleared both times.  Tests and A/B runs only."""

    def __init__(self, entry, value, caches=()):
        self.entry, self.value, self.caches = entry, int(value), caches

    def _set(self, value):
        prev = int(getattr(_lib.load(), self.entry)(value))
        for c in self.caches:
            c.clear()
        return prev

    def __enter__(self):
        self.prev = self._set(self.value)
        return self

    def __exit__(self, *a):
        self._set(self.prev)


def p8_conv(on=True):
    """Inside: 3x3 convs run on the 8-phase kernel (on=True) or the ring kernel (vst_p8_conv)."""
    return _Toggle("vst_p8_conv", bool(on))


def p8_persist(on=True):
    """Inside: the 8-phase GEMM's persistent grid is on / off (vst_p8_persist); the outputs are the same bits."""
    return _Toggle("vst_p8_persist", bool(on))


def sa_self(on=True):
    """Inside: the long self-attention runs on sa_self_kernel (on=True, the default) or on the general spatial kernel
    (vst_sa_self); the outputs are the same bits."""
    return _Toggle("vst_sa_self", bool(on))


def p8_tile_width(bn):
    """Inside: the 8-phase GEMM's tile width is forced (256 / 192 / 320 where legal; 0 = the library's policy)
    (vst_p8_force_bn)."""
    return _Toggle("vst_p8_force_bn", bn, (_LORA_BN, _XATTN_OK))


def gemm_lora_tile(M, N, K, P, group_n, group_r):
    """Tile width (256 / 192) of the in-GEMM LoRA projection (vst_gemm_lora) for this shape, 0 = not supported
    (the caller then runs the down-projection as its own pass).  Host-side policy only; no launch."""
    key = (M, N, K, P, group_n, group_r)
    bn = _LORA_BN.get(key)
    if bn is None:
        bn = _LORA_BN[key] = int(_lib.load().vst_gemm_lora_supported(M, N, K, P, group_n, group_r))
    return bn


def _gate(gate, gate_div, M, P, fn):
    """The row gate of the gated entries: an fp32 table of >= ceil(M / gate_div) rows x >= P columns (a single row of
    any stride).  Returns the three arguments the gated entries append."""
    if int(gate_div) <= 0:
        raise _lib.VstError(f"{fn}: gate_div {gate_div}")
    ld = _table(gate, (M + int(gate_div) - 1) // int(gate_div), P, "gate", fn, exact=False)
    return [_p(gate), ld, int(gate_div)]


def lora_gate(u: torch.Tensor, gate: torch.Tensor, gate_div: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[m, c] = bf16(gate[m // gate_div, c] * float(u[m, c])) (vst_lora_gate): the per-row content / style gate on
    an explicit LoRA down-projection u [M, P]; out may be u itself."""
    fn = "lora_gate"
    _view(u, BF16, "u", fn)
    M, P = u.shape
    g = _gate(gate, gate_div, M, P, fn)
    out = _new(out, (M, P), u, "out", fn)
    with _Rec("lora_gate", 1.0 * M * P, 4.0 * M * P, lambda: "lora_gate", (M, P)):
        _lib.call("vst_lora_gate", _p(u), _ld(u), M, P, *g, _p(out), _ld(out), _stream())
    return out


def linear_lora(x: torch.Tensor, w: torch.Tensor, a: torch.Tensor, group_n: int, group_r: int,
                bias: torch.Tensor | None = None, *, residual: torch.Tensor | None = None,
                out: torch.Tensor | None = None, r_alg: int | None = None, gate: torch.Tensor | None = None,
                gate_div: int = 1) -> torch.Tensor:
    """out = [x | bf16(x @ a^T)] @ w^T + bias (+ residual), the down-projection computed inside the GEMM
    (vst_gemm_lora).  w: [N, K + P] = [W | V], a: [P, K]; output columns n use u columns of group n // group_n.
    gate (fp32 [ceil(M / gate_div), >= P]): row m's u column c is scaled by gate[m // gate_div, c] after its bf16
    rounding and rounded again (vst_gemm_lora_gated); the same tile as without."""
    fn = "linear_lora"
    _view(x, BF16, "x", fn)
    _view(w, BF16, "w", fn)
    _view(a, BF16, "a", fn)
    M, K = x.shape
    N = w.shape[0]
    P = a.shape[0]
    if a.shape[1] != K or w.shape[1] != K + P:
        raise _lib.VstError(f"linear_lora: x {tuple(x.shape)} a {tuple(a.shape)} w {tuple(w.shape)}")
    out = _new(out, (M, N), x, "out", fn)
    if bias is not None:
        _vec(bias, N, "bias", fn)
    if residual is not None:
        _view(residual, BF16, "residual", fn, shape=(M, N))
    gated = [] if gate is None else _gate(gate, gate_div, M, P, fn)
    bn = gemm_lora_tile(M, N, K, P, group_n, group_r)
    if not bn:
        raise _lib.VstError(f"linear_lora: shape M={M} N={N} K={K} P={P} groups ({group_n}, {group_r}) unsupported")
    r = P if r_alg is None else r_alg
    # algorithmic work: base + up-projection (as the unfused "gemm_lora" counts it) + the down-projection once
    flops = 2.0 * M * N * (K + r) + 2.0 * M * K * r
    nbytes = 2.0 * (M * K + N * (K + r) + r * K + M * N * (2 if residual is not None else 1))
    sym = f"gemm_p8<128x{bn},lora>" if bn == 320 else f"gemm_p8<256x{bn},lora>"
    if gated:
        sym = sym[:-1] + ",gate>"
    with _Rec("gemm_lora", flops, nbytes, lambda: sym, (M, N, K + P)):
        _lib.call("vst_gemm_lora_gated" if gated else "vst_gemm_lora", _p(x), _ld(x), _p(a), _ld(a), P, group_n,
                  group_r, _p(w), _ld(w), M, N, K, _p(bias), _p(residual), 0 if residual is None else _ld(residual),
                  _p(out), _ld(out), *gated, _stream())
    return out


def cross_attention_fusable(M, N, K, lora, P, group_n, group_r, Nq, Nk):
    """Whether vst_gemm_cross_attention runs attn2 (q projection + text cross-attention) as one launch for this shape
    (host policy only, no launch)."""
    key = (M, N, K, bool(lora), P, group_n, group_r, Nq, Nk)
    ok = _XATTN_OK.get(key)
    if ok is None:
        ok = _XATTN_OK[key] = bool(_lib.load().vst_gemm_cross_attention_supported(M, N, K, int(bool(lora)), P,
                                                                                   group_n, group_r, Nq, Nk))
    return ok


def linear_cross_attention(x: torch.Tensor, w: torch.Tensor, a: torch.Tensor | None, group_n: int, group_r: int,
                           bias: torch.Tensor | None, k: torch.Tensor, v: torch.Tensor, *, Nq: int, Nk: int,
                           kv_div: int, scale: float, out: torch.Tensor | None = None,
                           r_alg: int | None = None, gate: torch.Tensor | None = None,
                           gate_div: int = 1) -> torch.Tensor:
    """o = softmax(q_h k_h^T scale) v_h per head (head_dim 64) with q = [x | bf16(x a^T)] w^T + bias computed in the
    same launch (vst_gemm_cross_attention); k / v: [text_batches * Nk, N] views (row stride >= N), the text batch of
    frame f = (m // Nq) is f // kv_div.  gate / gate_div: the row gate of linear_lora on q's down-projection
    (vst_gemm_cross_attention_gated; needs a)."""
    fn = "linear_cross_attention"
    _view(x, BF16, "x", fn)
    _view(w, BF16, "w", fn)
    _view(k, BF16, "k", fn)
    _view(v, BF16, "v", fn)
    M, K = x.shape
    N = w.shape[0]
    P = 0 if a is None else a.shape[0]
    if a is not None:
        _view(a, BF16, "a", fn)
        if a.shape[1] != K or w.shape[1] != K + P:
            raise _lib.VstError(f"linear_cross_attention: x {tuple(x.shape)} a {tuple(a.shape)} w {tuple(w.shape)}")
    elif w.shape[1] != K:
        raise _lib.VstError(f"linear_cross_attention: x {tuple(x.shape)} w {tuple(w.shape)}")
    if k.shape != v.shape or k.shape[1] != N or k.shape[0] % Nk or _ld(k) != _ld(v):
        raise _lib.VstError(f"linear_cross_attention: k {tuple(k.shape)} v {tuple(v.shape)} N={N} Nk={Nk}")
    if M % Nq or (M // Nq - 1) // kv_div >= k.shape[0] // Nk:
        raise _lib.VstError(f"linear_cross_attention: M={M} Nq={Nq} kv_div={kv_div} vs {k.shape[0] // Nk} text rows")
    if bias is not None:
        _vec(bias, N, "bias", fn)
    gated = []
    if gate is not None:
        if a is None:
            raise _lib.VstError("linear_cross_attention: a gate needs the LoRA operand a")
        gated = _gate(gate, gate_div, M, P, fn)
    if not cross_attention_fusable(M, N, K, a is not None, P, group_n, group_r, Nq, Nk):
        raise _lib.VstError(f"linear_cross_attention: M={M} N={N} K={K} Nq={Nq} Nk={Nk} not fusable")
    out = _new(out, (M, N), x, "out", fn)
    r = P if r_alg is None else r_alg
    flops = 2.0 * M * N * (K + r) + 2.0 * M * K * r + 4.0 * M * N * Nk
    nbytes = 2.0 * (M * K + N * (K + r) + r * K + 2 * (k.shape[0]) * N + M * N)
    sym = "gemm_p8<256x192,lora,xattn>" if a is not None else "gemm_p8<256x192,xattn>"
    if gated:
        sym = "gemm_p8<256x192,lora,gate,xattn>"
    with _Rec("gemm_xattn", flops, nbytes, lambda: sym, (M, N, K + P)):
        _lib.call("vst_gemm_cross_attention_gated" if gated else "vst_gemm_cross_attention", _p(x), _ld(x), _p(a),
                  0 if a is None else _ld(a), P, group_n, group_r, _p(w), _ld(w), _p(bias), M, N, K, _p(k), _p(v),
                  _ld(k), k.shape[0], Nq, Nk, kv_div, float(scale), _p(out), _ld(out), *gated, _stream())
    return out


_TATTN_OK = {}


def temporal_attention_fusable(M: int, K: int, nclip: int, F: int, HW: int, heads: int, head_dim: int) -> bool:
    """vst_gemm_temporal_attention_supported (host policy, cached): the motion modules' q/k/v + frame attention in one
    launch (16 frames, heads of 40)."""
    key = (M, K, nclip, F, HW, heads, head_dim)
    ok = _TATTN_OK.get(key)
    if ok is None:
        ok = _TATTN_OK[key] = bool(_lib.load().vst_gemm_temporal_attention_supported(*key))
    return ok


def temporal_qkv_layout(w: torch.Tensor, b: torch.Tensor | None, heads: int, head_dim: int):
    """The fused q/k/v weight [3C, K] (+ bias [3C]) re-laid out for vst_gemm_temporal_attention: per group of
    hpt = 256 // (3 head_dim) heads (2 of 40, 1 of 80) [q k v of each head] then zero rows up to 256.
    Returns (w_t bf16, b_t fp32)."""
    C = heads * head_dim
    hpt = 256 // (3 * head_dim)
    if w.shape[0] != 3 * C or hpt == 0 or heads % hpt:
        raise _lib.VstError(f"temporal_qkv_layout: w {tuple(w.shape)} heads={heads} head_dim={head_dim}")
    d = torch.arange(head_dim, device=w.device)
    rows, valid = [], []
    for t in range(heads // hpt):
        for h in range(hpt * t, hpt * t + hpt):
            for part in range(3):
                rows.append(part * C + h * head_dim + d)
        pad = 256 - 3 * hpt * head_dim
        rows.append(torch.zeros(pad, dtype=torch.long, device=w.device))
        valid.append(torch.cat([torch.ones(3 * hpt * head_dim, device=w.device), torch.zeros(pad, device=w.device)]))
    idx = torch.cat(rows)
    keep = torch.cat(valid)
    w_t = (w.detach().float()[idx] * keep[:, None]).to(BF16).contiguous()
    b_t = None if b is None else (b.detach().float()[idx] * keep).contiguous()
    return w_t, b_t


def linear_temporal_attention(x: torch.Tensor, w_t: torch.Tensor, b_t: torch.Tensor | None, *, nclip: int, F: int,
                              HW: int, heads: int, head_dim: int, scale: float,
                              out: torch.Tensor | None = None) -> torch.Tensor:
    """o = the motion modules' frame-axis attention of q/k/v = x w^T + b, in one launch (vst_gemm_temporal_attention);
    x: [nclip*F*HW, K] rows (clip, frame, pixel), w_t / b_t from temporal_qkv_layout.  Returns [M, heads*head_dim]."""
    fn = "linear_temporal_attention"
    _view(x, BF16, "x", fn)
    M, K = x.shape
    N = heads // (256 // (3 * head_dim)) * 256
    _view(w_t, BF16, "w_t", fn, shape=(N, K))
    if b_t is not None:
        _vec(b_t, N, "b_t", fn)
    if not temporal_attention_fusable(M, K, nclip, F, HW, heads, head_dim):
        raise _lib.VstError(f"linear_temporal_attention: M={M} K={K} F={F} HW={HW} heads={heads} not fusable")
    C = heads * head_dim
    out = _new(out, (M, C), x, "out", fn)
    flops = 2.0 * M * 3 * C * K + 4.0 * M * F * C
    nbytes = 2.0 * (M * K + 3 * C * K + M * C)
    with _Rec("gemm_tattn", flops, nbytes, lambda: "gemm_p8<256x256,tattn>", (M, N, K)):
        _lib.call("vst_gemm_temporal_attention", _p(x), _ld(x), _p(w_t), _ld(w_t), _p(b_t), M, K, nclip, F, HW, heads,
                  head_dim, float(scale), _p(out), _ld(out), _stream())
    return out


def _conv_in(x, rows, name, fn):
    """A conv input: the kernels address it as one contiguous [nimg*H*W, C] bf16 block."""
    _view(x, BF16, name, fn, rows=rows)
    if not x.is_contiguous():
        _fail(fn, name, f"must be contiguous [nimg*H*W, C], got stride {x.stride()}")
    return x.shape[1]


def conv3x3(x1: torch.Tensor, nimg: int, H: int, W: int, w: torch.Tensor, bias: torch.Tensor | None, *,
            x2: torch.Tensor | None = None, stride: int = 1, upsample: bool = False,
            row_bias: torch.Tensor | None = None, row_bias_div: int = 1, residual: torch.Tensor | None = None,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """NHWC 3x3 conv (pad 1).  x1: [nimg*H*W, C1] (+ x2: [nimg*H*W, C2] concatenated on channels).
    w: [Cout, 9*(C1+C2)] laid out (ky, kx, ci).  Returns [nimg*OH*OW, Cout]."""
    fn = "conv3x3"
    C1 = _conv_in(x1, nimg * H * W, "x1", fn)
    C2 = 0 if x2 is None else _conv_in(x2, nimg * H * W, "x2", fn)
    _view(w, BF16, "w", fn)
    Cout = w.shape[0]
    kreal = 9 * (C1 + C2)
    if w.shape[1] != ((kreal + 7) & ~7) and w.shape[1] != kreal:
        raise _lib.VstError(f"conv3x3: weight {tuple(w.shape)} vs K={kreal}")
    if upsample:
        OH, OW = 2 * H, 2 * W
    elif stride == 2:
        OH, OW = (H + 1) // 2, (W + 1) // 2
    else:
        OH, OW = H, W
    M = nimg * OH * OW
    out = _new(out, (M, Cout), x1, "out", fn)
    if bias is not None:
        _vec(bias, Cout, "bias", fn)
    if residual is not None:
        _view(residual, BF16, "residual", fn, shape=(M, Cout))
    ldrb = 0
    if row_bias is not None:
        if row_bias_div <= 0:
            raise _lib.VstError(f"conv3x3: row_bias_div {row_bias_div}")
        ldrb = _table(row_bias, (M - 1) // row_bias_div + 1, Cout, "row_bias", fn, align=False)
    kind = "conv3x3" if (C1 + C2) % 64 == 0 else "conv3x3_small_cin"
    with _Rec(kind, 2.0 * M * Cout * kreal, 2.0 * (nimg * H * W * (C1 + C2) + Cout * kreal + M * Cout),
              lambda: gemm_kernel_name(M, Cout, w.shape[1], 2 if kind == "conv3x3" else 3), (M, Cout, w.shape[1])):
        ws = _workspace(x1.device)
        _lib.call("vst_conv3x3_ex", _p(x1), C1, _p(x2), C2, nimg, H, W, stride, 1 if upsample else 0, _p(w), Cout,
                  _p(bias), _p(row_bias), row_bias_div, ldrb, _p(residual), 0 if residual is None else _ld(residual),
                  _p(out), _ld(out) if Cout >= 8 else Cout, GEMM_POLICY["tile"], _splits(), _p(ws),
                  _WS_BYTES, _stream())
    return out


FOLD_ROW_ALIGN = 256  # rows of one output-parity class are padded to this in the folded conv's GEMM (kFoldRowAlign)


def fold_upsample_weight(w: torch.Tensor) -> torch.Tensor:
    """The 3x3 kernel weight [Cout, 9C] (ky, kx, ci) folded for conv3x3_up_folded: [4*Cout, 4C], rows (class 2 py + px,
    co), columns (a, b, ci), each the fp32 sum of the taps that coincide in the nearest-2x upsampled image, rounded
    once to bf16 (vst_fold_upsample_weight)."""
    fn = "fold_upsample_weight"
    _block(w, BF16, "w", fn)
    if w.dim() != 2 or w.shape[1] % 72:
        _fail(fn, "w", f"must be [Cout, 9C] with C % 8 == 0, got {tuple(w.shape)}")
    Cout, C = w.shape[0], w.shape[1] // 9
    wf = torch.empty((4 * Cout, 4 * C), dtype=BF16, device=w.device)
    with _Rec("fold_upsample_weight", 7.0 * Cout * 4 * C, 2.0 * (9 + 16) * Cout * C, lambda: "fold_upsample_weight",
              (4 * Cout, 4 * C, 1)):
        _lib.call("vst_fold_upsample_weight", _p(w), Cout, C, _p(wf), _stream())
    return wf


def conv3x3_up_folded_applies(C: int, Cout: int) -> bool:
    """Shapes vst_conv3x3_up_folded takes (a shape-only answer: never the number of images)."""
    return C % 64 == 0 and Cout % 8 == 0


def conv3x3_up_folded(x: torch.Tensor, nimg: int, H: int, W: int, wf: torch.Tensor, bias: torch.Tensor | None, *,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """NHWC nearest-2x upsample + 3x3 conv (pad 1) as four 2x2 convs on the folded weight wf = fold_upsample_weight(w).
    x: [nimg*H*W, C] row view, C % 64 == 0.  Returns [nimg*2H*2W, Cout]; equal to conv3x3(upsample=True) up to the one
    rounding of the folded weights, at 4/9 of its multiply-adds."""
    fn = "conv3x3_up_folded"
    _view(x, BF16, "x", fn, rows=nimg * H * W)
    _view(wf, BF16, "wf", fn)
    C = x.shape[1]
    if wf.shape[0] % 4 or wf.shape[1] != 4 * C:
        _fail(fn, "wf", f"shape {tuple(wf.shape)}: expected [4*Cout, 4*C] with C = {C}")
    Cout = wf.shape[0] // 4
    if not conv3x3_up_folded_applies(C, Cout):
        raise _lib.VstError(f"conv3x3_up_folded: C={C} Cout={Cout} (needs C % 64 == 0, Cout % 8 == 0)")
    M = nimg * 4 * H * W
    out = _new(out, (M, Cout), x, "out", fn)
    if bias is not None:
        _vec(bias, Cout, "bias", fn)
    # the executed work: four padded classes of nimg*H*W rows, K = 4C
    rows = (nimg * H * W + FOLD_ROW_ALIGN - 1) // FOLD_ROW_ALIGN * FOLD_ROW_ALIGN
    with _Rec("conv3x3", 2.0 * M * Cout * 4 * C, 2.0 * (nimg * H * W * C + 4 * Cout * 4 * C + M * Cout),
              lambda: gemm_kernel_name(4 * rows, Cout, 4 * C, 4), (M, Cout, 4 * C)):
        _lib.call("vst_conv3x3_up_folded", _p(x), _ld(x), C, None, 0, nimg, H, W, _p(wf), _ld(wf), Cout, _p(bias),
                  None, None, _p(out), _ld(out), _stream())
    return out


def spatial_attention(q, k, v, nbatch, heads, Nq, Nk, kv_div=1, out=None, scale=None, lse=None):
    """q: [nbatch*Nq, >=heads*64] view; k/v: [nbatch/kv_div*Nk, >=heads*64] views.  lse: optional fp32
    [nbatch*heads*Nq] output of the log2-domain logsumexp per query (the training backward recomputes P from it)."""
    fn = "spatial_attention"
    _qkv(fn, q, k, v, nbatch * Nq, (nbatch // kv_div) * Nk)
    out = _new(out, (nbatch * Nq, heads * 64), q, "out", fn)
    if lse is not None:
        _block(lse, F32, "lse", fn, numel=nbatch * heads * Nq)
    scale = 0.125 if scale is None else scale
    with _Rec("spatial_attention", 4.0 * nbatch * heads * Nq * Nk * 64,
              2.0 * 64 * heads * (2 * nbatch * Nq + 2 * (nbatch // kv_div) * Nk), None, (nbatch * heads, Nq, Nk)):
        _lib.call("vst_spatial_attention", _p(q), _ld(q), _p(k), _p(v), k.stride(0), _p(out), _ld(out), nbatch,
                  heads, Nq, Nk, kv_div, 64, float(scale), _p(lse), _stream())
    return out


def frame_source(src) -> int:
    """The scalar the C ABI takes for one cross-frame source: "first" -> 0, "prev" -> -2, a frame index -> itself."""
    if src == "first":
        return 0
    if src == "prev":
        return -2
    if isinstance(src, bool) or not isinstance(src, int) or src < 0:
        raise ValueError(f"cross-frame source {src!r}: expected \"first\", \"prev\" or a frame index >= 0")
    return src


def frame_list(f: int, F: int, sources) -> list[int]:
    """Key/value frames of query frame f of an F-frame clip under `sources` (DESIGN.md "Cross-frame spatial
    self-attention"): [f, src1(f), src2(f)] with "prev" = max(f - 1, 0), minus every entry equal to an earlier one."""
    if not 0 <= f < F:
        raise ValueError(f"frame {f} outside 0..{F - 1}")
    out = [f]
    for src in sources:
        s = frame_source(src)
        if s >= F:
            raise ValueError(f"cross-frame source {s} >= F = {F}")
        s = max(f - 1, 0) if s == -2 else s
        if s not in out:
            out.append(s)
    return out


def spatial_attention_frames(q, k, v, nclip, F, heads, N, sources, scale=None, out=None):
    """Cross-frame spatial self-attention, head_dim 64: rows (b*F + f)*N + p; frame f of a clip attends to the tokens
    of frame_list(f, F, sources) of the same clip under one softmax.  q/k/v: [nclip*F*N, >= heads*64] views (k and v
    share a row stride); sources: up to two of "first", "prev" or a frame index.  Bad sources reach the library, which
    refuses them before any launch (VstError, status 1)."""
    fn = "spatial_attention_frames"
    rows = nclip * F * N
    _qkv(fn, q, k, v, rows)
    src = [frame_source(s) for s in sources]
    if len(src) > 2:
        raise _lib.VstError(f"spatial_attention_frames: {len(src)} sources; at most two")
    src1, src2 = (src + [-1, -1])[:2]
    out = _new(out, (rows, heads * 64), q, "out", fn)
    scale = 0.125 if scale is None else scale
    ok = all(s < F for s in src) and len(set(src)) == len(src)  # else the library refuses; nothing to count
    keys = sum(len(frame_list(f, F, sources)) for f in range(F)) * N if ok else 0
    with _Rec("spatial_attention_frames", 4.0 * 64 * heads * N * nclip * keys, 2.0 * 64 * heads * 4 * rows,
              lambda: "sa_frames_kernel", (nclip * F * heads, N, keys // F)):
        _lib.call("vst_spatial_attention_frames", _p(q), _ld(q), _p(k), _p(v), k.stride(0), _p(out), _ld(out), nclip,
                  F, heads, N, src1, src2, 64, float(scale), _stream())
    return out


def frame_adain(x, nclip, F, N, anchor, eps=1e-5, stats=None):
    """StyleAligned AdaIN to the anchor frame, in place (vst_frame_adain): x [nclip*F*N, C] bf16 view,
    rows (b*F + f)*N + p; every frame f != anchor of a clip becomes (x - mu_f) * (sd_a / sd_f) + mu_a per column, with
    the mean and the unbiased sd (eps inside the root) over the frame's N tokens; the anchor's rows are not written.
    stats: fp32 [nclip*F, 2, C] (mean row, sd row per frame), allocated when not given; written for every frame and
    returned.  F == 1 writes the statistics and leaves x alone."""
    fn = "frame_adain"
    nclip, F, N, anchor, eps = int(nclip), int(F), int(N), int(anchor), float(eps)
    if nclip < 1 or F < 1:
        _fail(fn, "nclip, F", f"= {nclip}, {F}: expected positive counts")
    if N < 2:
        _fail(fn, "N", f"= {N}: the unbiased variance needs at least 2 tokens per frame")
    if not 0 <= anchor < F:
        _fail(fn, "anchor", f"= {anchor}: outside the clip's frames 0..{F - 1}")
    if not 0.0 <= eps < float("inf"):
        _fail(fn, "eps", f"= {eps}: expected a finite value >= 0")
    _view(x, BF16, "x", fn, rows=nclip * F * N)
    C = x.shape[1]
    if C == 0 or C % 8 or _ld(x) % 8 or x.data_ptr() % 16:
        _fail(fn, "x", f"needs a multiple of 8 columns, a row stride that is a multiple of 8 and a 16-byte aligned "
                       f"base, got shape {tuple(x.shape)} stride {x.stride()}")
    if stats is None:
        stats = torch.empty((nclip * F, 2, C), dtype=F32, device=x.device)
    else:
        _block(stats, F32, "stats", fn, shape=(nclip * F, 2, C))
        if stats.data_ptr() % 16:
            _fail(fn, "stats", "needs a 16-byte aligned base")
    rows, moved = nclip * F * N, nclip * (F - 1) * N
    # statistics: one add, then subtract + fma per element; apply: subtract + fma.  HBM: x once for the statistics
    # (their second read is the L2's), once more and back for the apply; the statistics out and in again.
    nbytes = 2.0 * (rows + 2 * moved) * C + 8.0 * nclip * (3 * F - 2) * C
    with _Rec("frame_adain", (4.0 * rows + 3.0 * moved) * C, nbytes,
              lambda: "frame_adain_stats_kernel+frame_adain_apply_kernel", (nclip * F, N, C)):
        _lib.call("vst_frame_adain", _p(x), _ld(x), nclip, F, N, C, anchor, eps, _p(stats), _stream())
    return stats


def ip_attention_add(x, G, gbias, V, out, *, Nq, heads, T, kv_div=1, scale=0.125, layer_scale=1.0, row_scale=None):
    """IP-Adapter image attention added in place onto the attn2 output (vst_ip_attention_add).
    x [M, K] bf16: the hidden states attn2's to_q reads; G [nbatch*heads*16, K] bf16: the image keys folded into the
    query projection, 16 rows per (token batch, head) of which the first T count; gbias fp32 [nbatch*heads*16] or None:
    their product with to_q's bias; V [nbatch*16, 64*heads] bf16: the image values, 16 rows per token batch; out
    [M, 64*heads] bf16: the text attention's output, updated as
    out + layer_scale * row_scale[m // Nq] * softmax_t(scale * (x . G + gbias)) V.  Frame f = m // Nq reads token batch
    f // kv_div; row_scale fp32 [M // Nq] or None (= 1): a frame whose product with layer_scale is 0 is not written."""
    fn = "ip_attention_add"
    Nq, heads, T, kv_div = int(Nq), int(heads), int(T), int(kv_div)
    if Nq < 1 or heads < 1 or kv_div < 1:
        _fail(fn, "Nq, heads, kv_div", f"= {Nq}, {heads}, {kv_div}: expected positive counts")
    if not 1 <= T <= 16:
        _fail(fn, "T", f"= {T}: the kernel holds 1 to 16 image tokens")
    _view(x, BF16, "x", fn)
    M, K = x.shape
    if M == 0 or K == 0 or K % 64 or _ld(x) % 8 or x.data_ptr() % 16:
        _fail(fn, "x", f"needs rows, a multiple of 64 columns, a row stride that is a multiple of 8 and a 16-byte "
                       f"aligned base, got shape {tuple(x.shape)} stride {x.stride()}")
    if M % Nq:
        _fail(fn, "x", f"has {M} rows: not a multiple of Nq = {Nq}")
    nbatch = (M // Nq - 1) // kv_div + 1
    inner = 64 * heads

    def aligned(t, name):
        if _ld(t) % 8 or t.data_ptr() % 16:
            _fail(fn, name, f"needs a row stride that is a multiple of 8 and a 16-byte aligned base, got stride "
                            f"{t.stride()}")
    _view(G, BF16, "G", fn, min_cols=K)
    if G.shape[1] != K or G.shape[0] % (heads * 16) or G.shape[0] < nbatch * heads * 16:
        _fail(fn, "G", f"shape {tuple(G.shape)}: expected 16 rows of {K} columns per (token batch, head), "
                       f">= {nbatch} x {heads} of them")
    aligned(G, "G")
    nb = G.shape[0] // (heads * 16)
    _view(V, BF16, "V", fn, shape=(nb * 16, inner))
    aligned(V, "V")
    _view(out, BF16, "out", fn, shape=(M, inner))
    aligned(out, "out")
    if gbias is not None:
        _vec(gbias, nb * heads * 16, "gbias", fn)
        if gbias.data_ptr() % 16:
            _fail(fn, "gbias", "needs a 16-byte aligned base")
    if row_scale is not None:
        _vec(row_scale, M // Nq, "row_scale", fn)
    # scores 2 M heads 16 K, P.V 2 M heads 16 64 (the MFMAs run all 16 key rows); x once, O read and written, G, V
    flops = 2.0 * M * heads * 16 * (K + 64)
    nbytes = 2.0 * (M * K + 2 * M * inner + nb * heads * T * K + nb * T * inner)
    with _Rec("ip_attention_add", flops, nbytes, lambda: "ip_attention_add_kernel", (M, inner, K)):
        _lib.call("vst_ip_attention_add", _p(x), _ld(x), K, _p(G), _ld(G), _p(gbias), _p(V), _ld(V), nb, M, Nq, heads,
                  T, kv_div, float(scale), float(layer_scale), _p(row_scale), _p(out), _ld(out), _stream())
    return out


REGION_MAX = 4  # regions of vst_region_attention, the columns of its weight table


def region_attention(q, k, v, wts, *, nimg, heads, Nq, Nk, R, kv_div=1, scale=None, out=None):
    """Regional prompts: attn2 over R <= 4 prompts blended per query row (vst_region_attention).
    q [nimg*Nq, >= 64*heads] bf16 view; k / v [(nimg // kv_div)*R*Nk, >= 64*heads] bf16 views sharing a row stride,
    region r of token batch b at rows (b*R + r)*Nk; wts fp32 [nimg*Nq, 4], the normalised weights (columns >= R are
    not read).  out[m] = bf16(sum over r with wts[m, r] != 0 of wts[m, r] * softmax(q[m] K_r^T scale) V_r): a zero
    weight is a select, and a region that is zero on a whole 128-query block is not loaded there."""
    fn = "region_attention"
    nimg, heads, Nq, Nk, R, kv_div = int(nimg), int(heads), int(Nq), int(Nk), int(R), int(kv_div)
    if min(nimg, heads, Nq, Nk, kv_div) < 1:
        _fail(fn, "nimg, heads, Nq, Nk, kv_div", f"= {nimg}, {heads}, {Nq}, {Nk}, {kv_div}: expected positive counts")
    if not 1 <= R <= REGION_MAX:
        _fail(fn, "R", f"= {R}: the kernel blends 1 to {REGION_MAX} regions")
    if nimg % kv_div:
        _fail(fn, "nimg", f"= {nimg}: not a multiple of kv_div = {kv_div}")
    inner = 64 * heads
    _qkv(fn, q, k, v, nimg * Nq, (nimg // kv_div) * R * Nk)
    out = _new(out, (nimg * Nq, inner), q, "out", fn)
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.shape[1] < inner or _ld(t) % 8 or t.data_ptr() % 16:
            _fail(fn, name, f"needs >= {inner} columns, a row stride that is a multiple of 8 and a 16-byte aligned "
                            f"base, got shape {tuple(t.shape)} stride {t.stride()}")
    _block(wts, F32, "wts", fn, shape=(nimg * Nq, REGION_MAX))
    if wts.data_ptr() % 16:
        _fail(fn, "wts", "needs a 16-byte aligned base")
    scale = 0.125 if scale is None else scale
    # every region's scores and P.V for every row (an upper bound: dead regions are skipped); q, out, weights, K/V
    with _Rec("region_attention", 4.0 * nimg * heads * Nq * R * Nk * 64,
              2.0 * inner * (2 * nimg * Nq + 2 * (nimg // kv_div) * R * Nk) + 16.0 * nimg * Nq,
              lambda: "region_attn_kernel", (nimg * heads, Nq, R * Nk)):
        _lib.call("vst_region_attention", _p(q), _ld(q), _p(k), _p(v), k.stride(0), _p(wts), _p(out), _ld(out), nimg,
                  heads, Nq, Nk, R, kv_div, float(scale), _stream())
    return out


def temporal_attention(q, k, v, nclip, F, HW, heads, head_dim, out=None, scale=None):
    """Frame-axis attention; rows (b*F + f)*HW + p.  q/k/v views share one row stride."""
    fn = "temporal_attention"
    T = nclip * F * HW
    _qkv(fn, q, k, v, T, q_shares=True)
    out = _new(out, (T, heads * head_dim), q, "out", fn)
    scale = head_dim ** -0.5 if scale is None else scale
    with _Rec("temporal_attention", 4.0 * T * F * heads * head_dim, 2.0 * 4 * T * heads * head_dim):
        _lib.call("vst_temporal_attention", _p(q), _p(k), _p(v), q.stride(0), _p(out), _ld(out), nclip, F, HW, heads,
                  head_dim, float(scale), _stream())
    return out


def context_windows(F: int, L: int, S: int) -> list[int]:
    """Start frames of the sliding windows over an F-frame clip: 0, S, 2S, ... while start + L <= F, plus F - L when
    the last of those does not end the clip (every window L frames long, every frame covered); [0] when F <= L."""
    F, L, S = int(F), int(L), int(S)
    if not 1 <= L <= 32:
        raise ValueError(f"context_length {L} outside 1..32")
    if not 1 <= S <= L:
        raise ValueError(f"context_stride {S} outside 1..context_length ({L})")
    if F < 1:
        raise ValueError(f"F = {F}")
    if F <= L:
        return [0]
    starts = list(range(0, F - L + 1, S))
    if starts[-1] != F - L:
        starts.append(F - L)
    return starts


WEIGHTINGS = {"flat": 0, "pyramid": 1}


def context_weights(L: int, weighting: str = "pyramid") -> list[float]:
    """Blend weight of every window position: flat 1, pyramid min(j + 1, L - j)."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting {weighting!r} not in {sorted(WEIGHTINGS)}")
    if L < 1:
        raise ValueError(f"context_length {L}")
    return [float(min(j + 1, L - j)) if weighting == "pyramid" else 1.0 for j in range(L)]


def temporal_attention_windowed(q, k, v, pos, nclip, F, HW, heads, head_dim, context_length, context_stride,
                                weighting="pyramid", out=None, scale=None):
    """Frame-axis attention inside sliding windows of context_length frames, blended per frame (DESIGN.md "Long
    clips"); rows (b*F + f)*HW + p.  q/k/v views share one row stride and hold the projections WITHOUT the positional
    term; pos: fp32 [context_length, 3*heads*head_dim] = pe[:L] @ Wqkv^T (its q | k | v column blocks are added at the
    position inside each window), or None."""
    fn = "temporal_attention_windowed"
    L, S, C = int(context_length), int(context_stride), heads * head_dim
    nwin = len(context_windows(F, L, S))
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting {weighting!r} not in {sorted(WEIGHTINGS)}")
    if F < L:
        raise _lib.VstError(f"temporal_attention_windowed: F = {F} < context_length {L}")
    T = nclip * F * HW
    _qkv(fn, q, k, v, T, q_shares=True)
    pq = pk = pv = None
    ldpos = 0
    if pos is not None:
        ldpos = _table(pos, L, 3 * C, "pos", fn)
        pq, pk, pv = pos[:, :C], pos[:, C:2 * C], pos[:, 2 * C:]
    out = _new(out, (T, C), q, "out", fn)
    scale = head_dim ** -0.5 if scale is None else scale
    with _Rec("temporal_attention_windowed", 4.0 * nclip * HW * nwin * L * L * C, 2.0 * 4 * T * C,
              lambda: "temporal_attn_windowed_kernel"):
        _lib.call("vst_temporal_attention_windowed", _p(q), _p(k), _p(v), q.stride(0), _p(pq), _p(pk), _p(pv), ldpos,
                  _p(out), _ld(out), nclip, F, HW, heads, head_dim, L, S, WEIGHTINGS[weighting], float(scale),
                  _stream())
    return out


def group_norm(x1, nsamples, rows_per_sample, groups, eps, gamma, beta, *, silu=False, x2=None, out=None):
    fn = "group_norm"
    rows = nsamples * rows_per_sample
    _view(x1, BF16, "x1", fn, rows=rows)
    C = x1.shape[1] + (0 if x2 is None else _view(x2, BF16, "x2", fn, rows=rows).shape[1])
    _vec(gamma, C, "gamma", fn)
    _vec(beta, C, "beta", fn)
    out = _new(out, (rows, C), x1, "out", fn)
    ws_bytes = _lib.load().vst_groupnorm_workspace_bytes(nsamples, rows_per_sample, groups, C)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=F32, device=x1.device)
    with _Rec("groupnorm", 0.0, 2.0 * 3 * x1.shape[0] * C):  # two reads + one write
        _lib.call("vst_groupnorm", _p(x1), _ld(x1), x1.shape[1], _p(x2), 0 if x2 is None else _ld(x2),
                  0 if x2 is None else x2.shape[1], nsamples, rows_per_sample, groups, float(eps), _p(gamma),
                  _p(beta), 1 if silu else 0, _p(out), _ld(out), _p(ws), _stream())
    return out


def group_norm_frame_partials(x, nframes, rows_per_frame, groups, *, out=None):
    """fp32 (sum, sumsq) chunk partials of every frame, [nframes, chunks, groups, 2] (vst_groupnorm_frame_partials):
    a frame's partials depend on that frame only, so the frame-sharded motion GroupNorm all-gathers them."""
    fn = "group_norm_frame_partials"
    _view(x, BF16, "x", fn, rows=nframes * rows_per_frame)
    C = x.shape[1]
    nck = int(_lib.load().vst_groupnorm_frame_chunks(rows_per_frame))
    if out is None:
        out = torch.empty((nframes, nck, groups, 2), dtype=F32, device=x.device)
    _block(out, F32, "out", fn, numel=nframes * nck * groups * 2)
    with _Rec("groupnorm", 0.0, 2.0 * x.shape[0] * C):
        _lib.call("vst_groupnorm_frame_partials", _p(x), _ld(x), C, nframes, rows_per_frame, groups, _p(out),
                  _stream())
    return out


def group_norm_apply_partials(x, nclips, frames_local, rows_per_frame, groups, eps, gamma, beta, part, nranks, *,
                              silu=False, out=None):
    """GroupNorm of this rank's rows (clips x frames_local frames) with statistics over all nranks * frames_local
    frames of each clip, merged in one fixed order from `part` = [nranks, nclips, frames_local, chunks, groups, 2]
    (the all-gather of every rank's group_norm_frame_partials; nranks = 1: the whole clip is here)."""
    fn = "group_norm_apply_partials"
    _view(x, BF16, "x", fn, rows=nclips * frames_local * rows_per_frame)
    C = x.shape[1]
    nck = int(_lib.load().vst_groupnorm_frame_chunks(rows_per_frame))
    _block(part, F32, "part", fn, numel=nranks * nclips * frames_local * nck * groups * 2)
    _vec(gamma, C, "gamma", fn)
    _vec(beta, C, "beta", fn)
    out = _new(out, (x.shape[0], C), x, "out", fn)
    ss = torch.empty(2 * nclips * C, dtype=F32, device=x.device)
    with _Rec("groupnorm", 0.0, 2.0 * 2 * x.shape[0] * C):
        _lib.call("vst_groupnorm_apply_partials", _p(x), _ld(x), C, nclips, frames_local, rows_per_frame, groups,
                  _p(part), nranks, float(eps), _p(gamma), _p(beta), 1 if silu else 0, _p(out), _ld(out), _p(ss),
                  _stream())
    return out


def permute_rows(src, dims, perm, out=None):
    """src rows indexed (i0,i1,i2,i3) over `dims`; returns rows in order (i_perm[0], .., i_perm[3])."""
    fn = "permute_rows"
    _block(src, BF16, "src", fn)
    if src.dim() != 2 or src.shape[0] != dims[0] * dims[1] * dims[2] * dims[3]:
        raise _lib.VstError("permute_rows: src must be contiguous with prod(dims) rows")
    if out is None:
        out = torch.empty_like(src)
    _block(out, BF16, "out", fn, src.shape)
    with _Rec("permute", 0.0, 2.0 * 2 * src.numel()):
        _lib.call("vst_permute_rows", _p(src), _p(out), src.shape[1], *dims, *perm, _stream())
    return out


def add_row_table(x, table, *, div=1, mod=1, out=None):
    """out[row] = x[row] + table[(row // div) % mod]; table fp32 [>= mod, C] on device."""
    fn = "add_row_table"
    _view(x, BF16, "x", fn)
    rows, C = x.shape
    table = _on_device(table, F32, "table", fn).contiguous()
    _table(table, mod, C, "table", fn, align=False)
    out = _new(out, (rows, C), x, "out", fn)
    with _Rec("add_row_table", 0.0, 2.0 * 2 * rows * C):
        _lib.call("vst_add_row_table", _p(x), _ld(x), C, rows, _p(table), div, mod, _p(out), _ld(out), _stream())
    return out


def unpack_tokens(src, out):
    """bf16 token rows ((b*F + f)*HW + p, C) -> fp32 out (B, C, F, H, W) (contiguous)."""
    fn = "unpack_tokens"
    _block(out, F32, "out", fn)
    if out.dim() != 5:
        raise _lib.VstError("unpack_tokens: out must be a contiguous fp32 (B, C, F, H, W) device tensor")
    B, C, F, H, W = out.shape
    _block(src, BF16, "src", fn, (B * F * H * W, C))
    _lib.call("vst_unpack_tokens", _p(src), B, C, F, H * W, _p(out), _stream())
    return out


def layer_norm_lora(x, gamma, beta, eps, A, *, r_alg=None, out=None, u=None):
    """(LN(x), LN(x) @ A^T) in one pass; A: bf16 [R, C] (R % 16 == 0, <= 64) — LayerNorm + UnZipLoRA down."""
    fn = "layer_norm_lora"
    _view(x, BF16, "x", fn)
    _view(A, BF16, "A", fn)
    rows, C = x.shape
    R = A.shape[0]
    if A.shape[1] != C or R % 16 or R > 64 or C % 32 or C > 1280 or not A.is_contiguous():
        raise _lib.VstError(f"layer_norm_lora: x {tuple(x.shape)} A {tuple(A.shape)}")
    _vec(gamma, C, "gamma", fn)
    _vec(beta, C, "beta", fn)
    out = _new(out, (rows, C), x, "out", fn)
    u = _new(u, (rows, R), x, "u", fn)
    with _Rec("layernorm_lora", 2.0 * rows * C * (r_alg or R), 2.0 * (2 * rows * C + rows * R)):
        _lib.call("vst_layernorm_lora", _p(x), _ld(x), C, rows, _p(gamma), _p(beta), float(eps), _p(A), R, _p(out),
                  _ld(out), _p(u), _ld(u), _stream())
    return out, u


def layer_norm(x, gamma, beta, eps=1e-5, *, pe=None, pe_div=1, pe_mod=1, out=None):
    fn = "layer_norm"
    _view(x, BF16, "x", fn)
    rows, C = x.shape
    _vec(gamma, C, "gamma", fn)
    _vec(beta, C, "beta", fn)
    if pe is not None and (pe_mod <= 0 or _table(pe, pe_mod, C, "pe", fn) != C):
        _fail(fn, "pe", f"must be contiguous rows of C = {C} for pe_mod = {pe_mod} > 0")
    out = _new(out, (rows, C), x, "out", fn)
    with _Rec("layernorm", 0.0, 2.0 * 2 * rows * C):
        _lib.call("vst_layernorm", _p(x), _ld(x), C, rows, _p(gamma), _p(beta), float(eps), _p(pe), pe_div, pe_mod,
                  _p(out), _ld(out), _stream())
    return out


def _step_counter(step_idx, fn):
    return _block(step_idx, I32, "step_idx", fn, (1,))


def timestep_embedding(t, n, dim, out, *, col0=0, per_row=1, step_idx=None, flip=True, shift=0.0):
    """diffusers Timesteps(dim, flip_sin_to_cos, shift): value i -> out[i // per_row, col0 + (i % per_row)*dim].
    With step_idx (the device step counter) every value is t[step_idx], t the schedule's timestep table."""
    fn = "timestep_embedding"
    _block(t, F32, "t", fn)
    if step_idx is not None:
        _step_counter(step_idx, fn)
    if n <= 0 or per_row <= 0 or col0 < 0 or t.numel() < (1 if step_idx is not None else n):
        raise _lib.VstError(f"timestep_embedding: t {tuple(t.shape)} for n={n} values, per_row={per_row} col0={col0}")
    _view(out, BF16, "out", fn, min_cols=col0 + per_row * dim)
    if out.shape[0] * per_row < n:
        _fail(fn, "out", f"has {out.shape[0]} rows for n={n} values, {per_row} per row")
    _lib.call("vst_timestep_embedding", _p(t), _p(step_idx), n, dim, 1 if flip else 0, float(shift), _p(out),
              _ld(out), col0, per_row, _stream())
    return out


def _elementwise(entry, out, *ins):
    """silu / add / quick_gelu address every operand as one flat bf16 block of the first input's size."""
    fn, n = entry[4:], ins[0].numel() if isinstance(ins[0], torch.Tensor) else None
    for name, t in (("out", out),) + tuple((f"input {i}", t) for i, t in enumerate(ins)):
        _block(t, BF16, name, fn, numel=n)
    _lib.call(entry, *map(_p, ins), _p(out), n, _stream())
    return out


def silu(x, out=None):
    return _elementwise("vst_silu", torch.empty_like(x) if out is None else out, x)


def add(a, b, out=None):
    return _elementwise("vst_add", torch.empty_like(a) if out is None else out, a, b)


def quick_gelu(x, out=None):
    """x * sigmoid(1.702 x) (the CLIP ViT-L/14 MLP activation); out may be x."""
    return _elementwise("vst_quick_gelu", torch.empty_like(x) if out is None else out, x)


# ---- SDXL text encoders (text_encoder.py) ----
def embed_tokens(ids, L, tok, pos):
    """fp32 [rows, C]: tok[ids[r]] + pos[r % L] (CLIPTextEmbeddings).  ids: int32 [rows] on the device, in range (the
    caller checks them against the vocabulary on the host); tok [vocab, C] and pos [>= L, C]: contiguous bf16."""
    fn = "embed_tokens"
    _block(ids, I32, "ids", fn)
    _block(tok, BF16, "tok", fn)
    if ids.dim() != 1 or tok.dim() != 2 or L <= 0 or ids.numel() == 0:
        raise _lib.VstError(f"embed_tokens: ids {tuple(ids.shape)} (1-D), tok {tuple(tok.shape)} (2-D), L={L}")
    C = tok.shape[1]
    _block(pos, BF16, "pos", fn)
    if pos.dim() != 2 or pos.shape[1] != C or pos.shape[0] < L:
        _fail(fn, "pos", f"shape {tuple(pos.shape)}: expected >= {L} rows of C = {C}")
    h = torch.empty((ids.numel(), C), dtype=F32, device=ids.device)
    _lib.call("vst_embed_tokens", _p(ids), ids.numel(), L, _p(tok), _p(pos), C, _p(h), C, _stream())
    return h


def residual_layer_norm(h, y, gamma, beta, eps):
    """(h + y fp32, LayerNorm of it bf16) (vst_residual_layernorm): h the fp32 residual stream [rows, C], y bf16
    [rows, C] or None."""
    fn = "residual_layer_norm"
    _view(h, F32, "h", fn)
    rows, C = h.shape
    if y is not None:
        _view(y, BF16, "y", fn, shape=(rows, C))
    _vec(gamma, C, "gamma", fn)
    _vec(beta, C, "beta", fn)
    ho = torch.empty((rows, C), dtype=F32, device=h.device)
    n = torch.empty((rows, C), dtype=BF16, device=h.device)
    _lib.call("vst_residual_layernorm", _p(h), _ld(h), _p(y), 0 if y is None else _ld(y), rows, C, _p(gamma),
              _p(beta), float(eps), _p(ho), C, _p(n), C, _stream())
    return ho, n


def causal_attention(q, k, v, nbatch, heads, N, head_dim=64, out=None, scale=None):
    """CLIPAttention: softmax(q k^T * scale + causal mask) v over the N tokens of each of nbatch sequences; q/k/v:
    [nbatch*N, >= heads*head_dim] views (k and v share a row stride)."""
    fn = "causal_attention"
    _qkv(fn, q, k, v, nbatch * N)
    out = _new(out, (nbatch * N, heads * head_dim), q, "out", fn)
    scale = head_dim ** -0.5 if scale is None else scale
    _lib.call("vst_causal_attention", _p(q), _ld(q), _p(k), _p(v), k.stride(0), _p(out), _ld(out), nbatch, heads, N,
              head_dim, float(scale), _stream())
    return out


def transpose(x, out=None):
    """bf16 [rows, cols] (row-major view) -> [cols, rows]."""
    _view(x, BF16, "x", "transpose")
    rows, cols = x.shape
    out = _new(out, (cols, rows), x, "out", "transpose")
    with _Rec("transpose", 0.0, 2.0 * 2 * rows * cols):
        _lib.call("vst_transpose", _p(x), _ld(x), rows, cols, _p(out), _ld(out), _stream())
    return out


def layer_norm_bwd(x, g, gamma, eps=1e-5, need_affine=True):
    """LayerNorm backward: (dx bf16 [rows, C], dgamma fp32 [C], dbeta fp32 [C]); need_affine=False (frozen
    affine) computes dx only and returns (dx, None, None)."""
    fn = "layer_norm_bwd"
    _view(x, BF16, "x", fn)
    rows, C = x.shape
    _view(g, BF16, "g", fn, shape=(rows, C))
    _vec(gamma, C, "gamma", fn)
    dx = torch.empty((rows, C), dtype=BF16, device=x.device)
    dgamma = dbeta = ws = None
    if need_affine:
        dgamma = torch.empty(C, dtype=F32, device=x.device)
        dbeta = torch.empty(C, dtype=F32, device=x.device)
        ws = torch.empty((_lib.load().vst_layernorm_bwd_workspace_bytes(C, rows) + 3) // 4, dtype=F32,
                         device=x.device)
    with _Rec("layernorm_bwd", 0.0, 2.0 * 3 * rows * C):
        _lib.call("vst_layernorm_bwd", _p(x), _ld(x), _p(g), _ld(g), C, rows, _p(gamma), float(eps), _p(dx), _ld(dx),
                  _p(dgamma), _p(dbeta), _p(ws), _stream())
    return dx, dgamma, dbeta


def group_norm_bwd(x, g, nsamples, rows_per_sample, groups, eps, gamma, beta, *, silu=False):
    """GroupNorm (+SiLU) backward: (dx bf16, dgamma fp32 [C], dbeta fp32 [C])."""
    fn = "group_norm_bwd"
    _view(x, BF16, "x", fn, rows=nsamples * rows_per_sample)
    rows, C = x.shape
    _view(g, BF16, "g", fn, shape=(rows, C))
    _vec(gamma, C, "gamma", fn)
    _vec(beta, C, "beta", fn)
    dx = torch.empty((rows, C), dtype=BF16, device=x.device)
    dgamma = torch.empty(C, dtype=F32, device=x.device)
    dbeta = torch.empty(C, dtype=F32, device=x.device)
    ws = torch.empty((_lib.load().vst_groupnorm_bwd_workspace_bytes(nsamples, rows_per_sample, groups, C) + 3) // 4,
                     dtype=F32, device=x.device)
    with _Rec("groupnorm_bwd", 0.0, 2.0 * 5 * rows * C):
        _lib.call("vst_groupnorm_bwd", _p(x), _ld(x), _p(g), _ld(g), C, nsamples, rows_per_sample, groups, float(eps),
                  _p(gamma), _p(beta), int(silu), _p(dx), _ld(dx), _p(dgamma), _p(dbeta), _p(ws), _stream())
    return dx, dgamma, dbeta


def colsum(x, out=None):
    """fp32 [N] column sums of a bf16 [M, N] row-major view (bias gradients), deterministic (vst_colsum).  The kernel
    reads 16-B chunks of 8 columns: a view whose width, row stride or base is not 8-column aligned is first copied
    into a zero-padded [M, ceil8(N)] buffer (the padding columns sum to zero and are dropped)."""
    _view(x, BF16, "x", "colsum")
    M, N = x.shape
    if out is None:
        out = torch.empty(N, dtype=F32, device=x.device)
    _block(out, F32, "out", "colsum", (N,))
    if N % 8 or _ld(x) % 8 or x.data_ptr() % 16:
        n8 = (N + 7) // 8 * 8
        xp = torch.zeros((M, n8), dtype=BF16, device=x.device)
        xp[:, :N].copy_(x)  # (stream-ordered scratch: no cached buffer, which a captured graph would alias)
        full = colsum(xp)
        out.copy_(full[:N])
        return out
    ws = torch.empty((_lib.load().vst_colsum_workspace_bytes(M, N) + 3) // 4, dtype=F32, device=x.device)
    with _Rec("colsum", 0.0, 2.0 * M * N):
        _lib.call("vst_colsum", _p(x), _ld(x), M, N, _p(out), _p(ws), _stream())
    return out


def geglu_bwd(p, g, out=None):
    """dp (32-interleaved like p) from p = the GEGLU projection output and g = dL/d(h * gelu(gate))."""
    _view(g, BF16, "g", "geglu_bwd")
    M, Nh = g.shape
    _view(p, BF16, "p", "geglu_bwd", shape=(M, 2 * Nh))
    out = _new(out, (M, 2 * Nh), p, "out", "geglu_bwd")
    with _Rec("geglu_bwd", 0.0, 2.0 * 5 * M * Nh):
        _lib.call("vst_geglu_bwd", _p(p), _ld(p), _p(g), _ld(g), M, Nh, _p(out), _ld(out), _stream())
    return out


def spatial_attention_bwd(q, k, v, o, dout, lse, nbatch, heads, Nq, Nk, kv_div=1, scale=None, dq=None, dkv=None,
                          need_dkv=True):
    """(dq [nbatch*Nq, heads*64], dk, dv [nbatch/kv_div*Nk, heads*64] as column views of one [.., 2*heads*64], or
    None, None when need_dkv is False: frozen K/V skip the dK/dV kernel).  lse: the forward's logsumexp output."""
    fn = "spatial_attention_bwd"
    C = heads * 64
    nkv = nbatch // kv_div
    _qkv(fn, q, k, v, nbatch * Nq, nkv * Nk, o=o, dout=dout)
    _block(lse, F32, "lse", fn, numel=nbatch * heads * Nq)
    dq = _new(dq, (nbatch * Nq, C), q, "dq", fn)
    dk = dv = None
    if need_dkv:
        dkv = _new(dkv, (nkv * Nk, 2 * C), q, "dkv", fn)
        dk, dv = dkv[:, :C], dkv[:, C:]
    ws = torch.empty((_lib.load().vst_spatial_attention_bwd_workspace_bytes(nbatch, heads, Nq, Nk) + 3) // 4,
                     dtype=F32, device=q.device)
    scale = 0.125 if scale is None else scale
    # MFMA work: dQ pass 3 products (S, dP, dQ), dK/dV pass 4 (S, dP, dV, dK), 2*64 flop per (q, key) each
    with _Rec("spatial_attention_bwd", (6.0 + (8.0 if need_dkv else 0.0)) * nbatch * heads * Nq * Nk * 64, 0.0):
        _lib.call("vst_spatial_attention_bwd", _p(q), _ld(q), _p(k), _p(v), k.stride(0), _p(o), _ld(o), _p(dout),
                  _ld(dout), _p(lse), _p(dq), _ld(dq), _p(dk), _p(dv), dkv.stride(0) if need_dkv else 0, nbatch,
                  heads, Nq, Nk, kv_div, 64, float(scale), _p(ws), _stream())
    return dq, dk, dv


def temporal_attention_bwd(q, k, v, dout, nclip, F, HW, heads, head_dim, scale=None, out=None):
    """(dq, dk, dv) of temporal_attention as column views of one [tokens, 3C] bf16 buffer."""
    fn = "temporal_attention_bwd"
    C = heads * head_dim
    rows = nclip * F * HW
    _qkv(fn, q, k, v, rows, q_shares=True, dout=dout)
    out = _new(out, (rows, 3 * C), q, "out", fn)
    scale = head_dim ** -0.5 if scale is None else scale
    with _Rec("temporal_attention_bwd", 0.0, 2.0 * 7 * rows * C):
        _lib.call("vst_temporal_attention_bwd", _p(q), _p(k), _p(v), q.stride(0), _p(dout), _ld(dout), _p(out[:, :C]),
                  _p(out[:, C:2 * C]), _p(out[:, 2 * C:]), out.stride(0), nclip, F, HW, heads, head_dim, float(scale),
                  _stream())
    return out[:, :C], out[:, C:2 * C], out[:, 2 * C:]


def _sampler_in(fn, x, rows):
    """The sampler dgrad kernels address x as one contiguous [rows, C] block of 16-byte chunks (no row stride in their
    ABI): a shorter, strided or misaligned x would be read past its end.  Returns C."""
    _block(x, BF16, "x", fn)
    if x.dim() != 2 or x.shape[0] != rows or rows <= 0 or x.shape[1] % 8 or x.data_ptr() % 16:
        _fail(fn, "x", f"must be a 16-byte aligned [{rows}, C % 8 == 0] block, got shape {tuple(x.shape)}")
    return x.shape[1]


def zero_insert(x, nimg, h, w):
    """[nimg*h*w, C] -> [nimg*2h*2w, C] with x on the even (2i, 2j) pixels, zeros elsewhere."""
    C = _sampler_in("zero_insert", x, nimg * h * w)
    out = torch.zeros((nimg * 4 * h * w, C), dtype=BF16, device=x.device)
    _lib.call("vst_zero_insert", _p(x), nimg, h, w, C, _p(out), _stream())
    return out


def sumpool2x2(x, nimg, h, w):
    """[nimg*2h*2w, C] -> [nimg*h*w, C], 2x2 block sums (h, w: output size)."""
    C = _sampler_in("sumpool2x2", x, nimg * 4 * h * w)
    out = torch.empty((nimg * h * w, C), dtype=BF16, device=x.device)
    _lib.call("vst_sumpool2x2", _p(x), nimg, h, w, C, _p(out), _stream())
    return out


def copy2d(x, out):
    _view(x, BF16, "x", "copy2d")
    _view(out, BF16, "out", "copy2d", shape=x.shape)
    _lib.call("vst_copy2d", _p(x), _ld(x), _p(out), _ld(out), x.shape[0], x.shape[1], _stream())
    return out


def pack_latents(lat, out, *, sigmas=None, step_idx=None, fixed_scale=1.0, ncopy=1):
    """fp32 latents (B, C, F, H, W) -> bf16 token rows out [ncopy*B*F*H*W, C] (each copy the same rows), scaled by
    fixed_scale, or with sigmas by 1 / sqrt(sigmas[step_idx]^2 + 1) read on the device."""
    fn = "pack_latents"
    _block(lat, F32, "lat", fn)
    if lat.dim() != 5 or lat.numel() == 0 or ncopy <= 0:
        raise _lib.VstError(f"pack_latents: latents must be (B,C,F,H,W), got {tuple(lat.shape)}; ncopy {ncopy}")
    B, Cl, F, H, W = lat.shape
    if sigmas is not None:
        _schedule(sigmas, step_idx, fn)
    elif step_idx is not None:
        _step_counter(step_idx, fn)
    _block(out, BF16, "out", fn, (ncopy * B * F * H * W, Cl))
    _lib.call("vst_pack_latents", _p(lat), B, Cl, F, H * W, _p(sigmas), _p(step_idx), float(fixed_scale), ncopy,
              _p(out), _stream())
    return out


def euler_cfg_step(noise, lat, sigmas, step_idx, *, guidance=7.5, ncopy=2):
    """lat += (sigmas[step + 1] - sigmas[step]) * e in place, e = u + guidance * (c - u) from the CFG pair's UNet
    output rows noise (ncopy 1: the only rows)."""
    B, Cl, F, H, W = _step_operands(noise, lat, sigmas, step_idx, ncopy, "euler_cfg_step")
    _lib.call("vst_euler_cfg_step", _p(noise), ncopy, float(guidance), _p(lat), B, Cl, F, H * W, _p(sigmas),
              _p(step_idx), _stream())


def step_advance(step_idx, num_steps):
    """step_idx <- (step_idx + 1) mod num_steps on the device (a schedule of num_steps steps)."""
    _lib.call("vst_step_advance", _p(_step_counter(step_idx, "step_advance")), int(num_steps), _stream())


# ---- FreeU in the up path (freeu.FreeU) ----
def freeu(x, skip, nimg, H, W, table, stage, *, x_out=None, skip_out=None):
    """diffusers' apply_freeu on token rows (vst_freeu): x [nimg*H*W, Cx] and skip [nimg*H*W, Cs] bf16 ->
    (x_out, skip_out) with x_out[:, :Cx/2] = bf16(x * b), the rest x's bits, and skip_out the skip with the four lowest
    frequency bins of every (image, channel) map scaled by s; (s, b) = table[stage], fp32 [2, 2] on the device (read
    there: new values replay a captured step).  x_out may be x (in place); skip_out must not overlap skip.  The
    GroupNorm that follows reads the filtered skip like any other tensor."""
    rows = nimg * H * W
    _view(x, BF16, "x", "freeu", rows=rows)
    _view(skip, BF16, "skip", "freeu", rows=rows)
    _block(table, F32, "table", "freeu", (2, 2))
    Cx, Cs = x.shape[1], skip.shape[1]
    x_out = _new(x_out, (rows, Cx), x, "x_out", "freeu")
    skip_out = _new(skip_out, (rows, Cs), x, "skip_out", "freeu")
    inplace = x_out.data_ptr() == x.data_ptr()
    nbytes = 4.0 * rows * Cs + 2.0 * rows * (Cx if inplace else 2 * Cx)
    with _Rec("freeu", 28.0 * rows * Cs, nbytes, lambda: "freeu_kernel", (rows, Cs, Cx)):
        _lib.call("vst_freeu", _p(x), _ld(x), Cx, _p(skip), _ld(skip), Cs, _p(x_out), _ld(x_out), _p(skip_out),
                  _ld(skip_out), nimg, H, W, _p(table), int(stage), _stream())
    return x_out, skip_out


# ---- video-to-video: start latents from a source clip, the masked Euler step (pipeline.set_source) ----
def _schedule(sigmas, step_idx, fn):
    _block(sigmas, F32, "sigmas", fn)
    _step_counter(step_idx, fn)
    if sigmas.dim() != 1 or sigmas.numel() < 2:
        raise _lib.VstError(f"{fn}: sigmas must be a 1-D table of num_steps + 1 entries, got {tuple(sigmas.shape)}")


def _step_operands(noise, lat, sigmas, step_idx, ncopy, fn):
    """What every denoise step takes: lat (B, Cl, F, H, W) fp32, ncopy 1 or 2, noise rows (ncopy * B * F * H * W, Cl)
    bf16, the sigma table and the step counter.  Returns lat's dimensions."""
    _block(lat, F32, "lat", fn)
    if lat.dim() != 5 or lat.numel() == 0:
        raise _lib.VstError(f"{fn}: lat must be (B, Cl, F, H, W), got {tuple(lat.shape)}")
    B, Cl, F, H, W = lat.shape
    if ncopy not in (1, 2):
        raise _lib.VstError(f"{fn}: ncopy {ncopy} (1 or 2)")
    _block(noise, BF16, "noise", fn, (ncopy * B * F * H * W, Cl))
    _schedule(sigmas, step_idx, fn)
    return B, Cl, F, H, W


def _keep_mask(lat, z0, eps, mask, fn):
    """The keep-mask triple of a step on lat: z0 and eps of lat's shape, mask (1 or B, F, H, W).  Returns mask_clips."""
    B, _, F, H, W = lat.shape
    _block(z0, F32, "z0", fn, lat.shape)
    _block(eps, F32, "eps", fn, lat.shape)
    _block(mask, F32, "mask", fn)
    if mask.dim() != 4 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (F, H, W):
        raise _lib.VstError(f"{fn}: mask {tuple(mask.shape)} vs (1 or {B}, {F}, {H}, {W})")
    return mask.shape[0]


def noise_latents(z0, eps, sigmas, step_idx, out=None):
    """fp32 z0 + sigmas[step_idx] * eps (the start latents of a source-clip run; sigma is read on the device)."""
    fn = "noise_latents"
    _block(z0, F32, "z0", fn)
    _block(eps, F32, "eps", fn, z0.shape)
    _schedule(sigmas, step_idx, fn)
    if z0.numel() == 0:
        raise _lib.VstError(f"{fn}: empty latents")
    if out is None:
        out = torch.empty_like(z0)
    _block(out, F32, "out", fn, z0.shape)
    _lib.call("vst_noise_latents", _p(z0), _p(eps), _p(sigmas), _p(step_idx), _p(out), z0.numel(), _stream())
    return out


def euler_cfg_step_masked(noise, lat, sigmas, step_idx, z0, eps, mask, *, guidance=7.5, ncopy=2):
    """euler_cfg_step, then lat = mask * lat + (1 - mask) * (z0 + sigmas[step + 1] * eps) in fp32: mask
    (1 or B, F, H, W) in [0, 1] over the channels of lat / z0 / eps (B, Cl, F, H, W); 1 = free, 0 = keep z0."""
    fn = "euler_cfg_step_masked"
    B, Cl, F, H, W = _step_operands(noise, lat, sigmas, step_idx, ncopy, fn)
    mask_clips = _keep_mask(lat, z0, eps, mask, fn)
    _lib.call("vst_euler_cfg_step_masked", _p(noise), ncopy, float(guidance), _p(lat), B, Cl, F, H * W, _p(sigmas),
              _p(step_idx), _p(z0), _p(eps), _p(mask), mask_clips, _stream())


# ---- few-step sampling: the table-driven sampler step and guidance rescale (pipeline._step) ----
def _sampler_operands(fn, noise, lat, hist, sigmas, coef, ncoef, step_idx, ncopy, factor, z0, eps, mask):
    """What sampler_step and sampler_step_noise share: the step operands, hist (never lat itself), the coefficient
    table [num_steps, ncoef], the optional rescale factor [B] and keep-mask triple.  Returns (B, Cl, F, H*W,
    mask_clips)."""
    B, Cl, F, H, W = _step_operands(noise, lat, sigmas, step_idx, ncopy, fn)
    _block(hist, F32, "hist", fn, lat.shape)
    if hist.data_ptr() == lat.data_ptr():
        raise _lib.VstError(f"{fn}: hist must not be lat")
    _block(coef, F32, "coef", fn, (sigmas.numel() - 1, ncoef))
    if factor is not None:
        _block(factor, F32, "factor", fn, (B,))
        if ncopy != 2:
            raise _lib.VstError(f"{fn}: a rescale factor needs both CFG branches (ncopy 2)")
    given = [t is not None for t in (z0, eps, mask)]
    if any(given) and not all(given):
        raise _lib.VstError(f"{fn}: z0, eps and mask go together")
    return B, Cl, F, H * W, _keep_mask(lat, z0, eps, mask, fn) if mask is not None else 0


def sampler_step(noise, lat, hist, sigmas, coef, step_idx, *, guidance=7.5, ncopy=2, factor=None, z0=None, eps=None,
                 mask=None):
    """One fused sampler step on lat and hist (B, Cl, F, H, W) fp32, in place: e = u + guidance * (c - u) (times
    factor[b] when given), D = lat - sigmas[s] * e, lat = a * lat + b * D + c * hist with (a, b, c) = coef[s]
    (scheduler.sampler_coefficients as fp32 [n, 3]), hist = D; with z0 / eps / mask (all three) the keep-mask blend of
    euler_cfg_step_masked follows.  hist is not read where c == 0."""
    B, Cl, F, HW, mask_clips = _sampler_operands("sampler_step", noise, lat, hist, sigmas, coef, 3, step_idx, ncopy,
                                                 factor, z0, eps, mask)
    _lib.call("vst_sampler_step", _p(noise), ncopy, float(guidance), _p(lat), _p(hist), B, Cl, F, HW, _p(sigmas),
              _p(coef), _p(step_idx), _p(factor), _p(z0), _p(eps), _p(mask), mask_clips, _stream())


# ---- stochastic samplers: counter-based noise and the step that adds it (pipeline._step) ----
def _noise_operands(seed, step_idx, stream_id, shape, F_total, f0, fn):
    """What every noise entry takes: the device seed (int64 [1], read as the uint64 of its bits) and step counter, a
    stream below 2^16, and a (B, Cl, F, H, W) shape holding frames [f0, f0 + F) of F_total.  Returns F_total."""
    _block(seed, torch.int64, "seed", fn, (1,))
    _step_counter(step_idx, fn)
    if len(shape) != 5 or min(shape) <= 0:
        raise _lib.VstError(f"{fn}: shape {tuple(shape)} must be (B, Cl, F, H, W), all positive")
    F_total = shape[2] if F_total is None else int(F_total)
    if not 0 <= int(stream_id) < 1 << 16 or shape[1] > 1 << 18:
        raise _lib.VstError(f"{fn}: stream_id {stream_id} must be in [0, 65535] and Cl {shape[1]} at most 2^18")
    if f0 < 0 or f0 + shape[2] > F_total:
        raise _lib.VstError(f"{fn}: frames [{f0}, {f0 + shape[2]}) outside the clip's {F_total}")
    return F_total


def _noise_fill(entry, dtype, seed, step_idx, shape, stream_id, F_total, f0, out):
    fn = entry[4:]
    shape = tuple(int(v) for v in shape)
    F_total = _noise_operands(seed, step_idx, stream_id, shape, F_total, f0, fn)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=seed.device)
    _block(out, dtype, "out", fn, shape)
    B, Cl, F, H, W = shape
    _lib.call(entry, _p(out), _p(seed), _p(step_idx), int(stream_id), B, Cl, F, F_total, int(f0), H * W, _stream())
    return out


def noise_bits(seed, step_idx, shape, *, stream_id=0, F_total=None, f0=0, out=None):
    """The Philox4x32-10 word of every element of a (B, Cl, F, H, W) tensor holding frames [f0, f0 + F) of clips of
    F_total frames (default F), as int32 bit patterns (view them as torch.uint32): scheduler.noise_reference's bits."""
    return _noise_fill("vst_noise_bits", I32, seed, step_idx, shape, stream_id, F_total, f0, out)


def noise_normal(seed, step_idx, shape, *, stream_id=0, F_total=None, f0=0, out=None):
    """fp32 standard normals of the same counters (Box-Muller on the words); stream_id 0 at step s is what
    sampler_step_noise adds at step s."""
    return _noise_fill("vst_noise_normal", F32, seed, step_idx, shape, stream_id, F_total, f0, out)


def sampler_step_noise(noise, lat, hist, sigmas, coef, step_idx, seed, *, F_total=None, f0=0, guidance=7.5, ncopy=2,
                       factor=None, z0=None, eps=None, mask=None):
    """sampler_step on coef rows (a, b, c, d) (scheduler.sampler_coefficients of a stochastic sampler, fp32 [n, 4]):
    lat = a * lat + b * D + c * hist + d * xi, xi = noise_normal(seed, step_idx, lat.shape, F_total=, f0=) generated in
    the kernel; the keep-mask blend follows.  Where d == 0 no noise is generated and lat has sampler_step's bits."""
    fn = "sampler_step_noise"
    B, Cl, F, HW, mask_clips = _sampler_operands(fn, noise, lat, hist, sigmas, coef, 4, step_idx, ncopy, factor, z0,
                                                 eps, mask)
    F_total = _noise_operands(seed, step_idx, 0, tuple(lat.shape), F_total, f0, fn)
    _lib.call("vst_sampler_step_noise", _p(noise), ncopy, float(guidance), _p(lat), _p(hist), B, Cl, F, F_total,
              int(f0), HW, _p(sigmas), _p(coef), _p(step_idx), _p(seed), _p(factor), _p(z0), _p(eps), _p(mask),
              mask_clips, _stream())


def cfg_rescale_workspace(lat_shape, device):
    """The fp32 workspace cfg_rescale_factor needs for latents of this (B, Cl, F, H, W) shape."""
    B, Cl, F, H, W = lat_shape
    nbytes = int(_lib.load().vst_cfg_rescale_factor_workspace_bytes(B, Cl, F, H * W))
    return torch.empty((nbytes + 3) // 4, dtype=F32, device=device)


def cfg_rescale_factor(noise, lat_shape, *, guidance, phi, out=None, workspace=None):
    """fp32 [B]: phi * std(cond_b) / std(e_b) + (1 - phi) per clip, e = u + guidance * (c - u), from the CFG pair's
    UNet output rows noise (2 * B * F * H * W, Cl) bf16 (1 where std(e_b) is 0).  The same bits on every call."""
    fn = "cfg_rescale_factor"
    if len(lat_shape) != 5 or min(lat_shape) <= 0:
        raise _lib.VstError(f"{fn}: latent shape {tuple(lat_shape)} must be (B, Cl, F, H, W), all positive")
    B, Cl, F, H, W = lat_shape
    _block(noise, BF16, "noise", fn, (2 * B * F * H * W, Cl))
    phi = float(phi)
    if not 0.0 <= phi <= 1.0:  # also refuses NaN
        raise _lib.VstError(f"{fn}: phi {phi} outside [0, 1]")
    if out is None:
        out = torch.empty(B, dtype=F32, device=noise.device)
    _block(out, F32, "out", fn, (B,))
    if workspace is None:
        workspace = cfg_rescale_workspace(lat_shape, noise.device)
    _block(workspace, F32, "workspace", fn)
    need = int(_lib.load().vst_cfg_rescale_factor_workspace_bytes(B, Cl, F, H * W))
    if workspace.numel() * 4 < need:
        raise _lib.VstError(f"{fn}: workspace of {workspace.numel() * 4} bytes, {need} needed")
    _lib.call("vst_cfg_rescale_factor", _p(noise), float(guidance), phi, B, Cl, F, H * W, _p(out), _p(workspace),
              _stream())
    return out


# ---- FreeInit: the frequency mix between two passes of the loop (free_init.FreeInit) ----
FREE_INIT_MAX_AXIS = 128  # the longest F, H or W vst_free_init_mix takes


def free_init_workspace_bytes(shape) -> int:
    """Bytes of the spectrum vst_free_init_mix keeps between its launches (the formula of include/vst.h)."""
    B, Cl, F, H, W = (int(v) for v in shape)
    return B * Cl * F * H * (W // 2 + 1) * 8


def free_init_workspace(shape, device):
    """The fp32 workspace free_init_mix needs for latents of this (B, Cl, F, H, W) shape."""
    if len(shape) != 5 or min(shape) <= 0:
        raise _lib.VstError(f"free_init_mix: shape {tuple(shape)} must be (B, Cl, F, H, W), all positive")
    return torch.empty(free_init_workspace_bytes(shape) // 4, dtype=F32, device=device)


def free_init_mix(x, init, filt, scale, *, noise=None, seed=None, it=None, stream_id=1, out=None, workspace=None):
    """FreeInit's mix on fp32 (B, Cl, F, H, W) latents (vst_free_init_mix): out = r + L(x + init - r), L the 3-D low-pass
    with filt = free_init.dft_order(mask) as fp32 [F, H, W]; init may be None.  r = scale * noise (noise of x's shape),
    or, with seed (int64 [1]) and it (int32 [1]) instead, scale * noise_normal(seed, it, x.shape, stream_id=stream_id),
    regenerated in the kernel and read on the device, so a captured launch replays with new values.  out may be x."""
    fn = "free_init_mix"
    _block(x, F32, "x", fn)
    if x.dim() != 5 or x.numel() == 0:
        raise _lib.VstError(f"{fn}: x must be (B, Cl, F, H, W), got {tuple(x.shape)}")
    B, Cl, F, H, W = x.shape
    if init is not None:
        _block(init, F32, "init", fn, x.shape)
    _block(filt, F32, "filt", fn, (F, H, W))
    if (noise is None) == (seed is None) or (seed is None) != (it is None):
        raise _lib.VstError(f"{fn}: give noise, or seed and it (one source of the fresh noise)")
    if noise is not None:
        _block(noise, F32, "noise", fn, x.shape)
    else:
        _noise_operands(seed, it, stream_id, tuple(x.shape), None, 0, fn)
    if out is None:
        out = torch.empty_like(x)
    _block(out, F32, "out", fn, x.shape)
    if workspace is None:
        workspace = free_init_workspace(x.shape, x.device)
    _block(workspace, F32, "workspace", fn)
    need = free_init_workspace_bytes(x.shape)
    if workspace.numel() * 4 < need:
        raise _lib.VstError(f"{fn}: workspace of {workspace.numel() * 4} bytes, {need} needed")
    n = x.numel()
    flops = 8.0 * B * Cl * F * H * (W // 2 + 1) * (W / 2 + 2 * H + 2 * F) + 2.0 * n * (W // 2)
    with _Rec("free_init_mix", flops, 4.0 * n * (3 if init is None else 4) + 4.0 * need, lambda: "mix_plane_fwd_kernel",
              tuple(x.shape)):
        _lib.call("vst_free_init_mix", _p(x), _p(init), _p(noise), _p(out), _p(filt), float(scale), _p(seed), _p(it),
                  int(stream_id), B, Cl, F, H, W, _p(workspace), workspace.numel() * 4, _stream())
    return out


# ---- token merging (token_merge.TokenMerging) ----
TOME_MAX_TOKENS = 4096  # the most tokens per image vst_tome_match takes
TOME_MAX_CHANNELS = 1280


def tome_sizes(H: int, W: int, sy: int, sx: int, ratio: float):
    """(N, Nd, Ns, r) of an H x W image cut into sy x sx cells: the tokens, the destinations (whole cells), the sources
    and the merged sources r = min(Ns, int(ratio * N))."""
    H, W, sy, sx = int(H), int(W), int(sy), int(sx)
    if min(H, W, sy, sx) < 1 or sy > H or sx > W:
        raise _lib.VstError(f"token merging: cells of {sy} x {sx} on a {H} x {W} image")
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:  # also refuses NaN
        raise _lib.VstError(f"token merging: ratio {ratio} outside [0, 1]")
    N = H * W
    Nd = (H // sy) * (W // sx)
    return N, Nd, N - Nd, min(N - Nd, int(ratio * N))


def tome_plan_ints(N: int) -> int:
    """int32 per image of a plan (the formula of include/vst.h)."""
    return 6 * int(N) + 4


def tome_plan(nimg: int, N: int, device):
    """A plan buffer for nimg images of N tokens (int32 [nimg, 6 N + 4]), zero-filled so that a merge before any match
    reads valid rows."""
    nbytes = int(_lib.load().vst_tome_plan_bytes(int(nimg), int(N), 0))
    if nbytes != nimg * tome_plan_ints(N) * 4:
        raise _lib.VstError(f"tome_plan: {nimg} images of {N} tokens")
    return torch.zeros((nimg, tome_plan_ints(N)), dtype=I32, device=device)


def _tome_operands(fn, x, nimg, H, W, sy, sx, r, plan, name="x", rows=None):
    """The operands the three token-merging entries share: a bf16 view of nimg * (rows or H * W) rows whose width is a
    multiple of 64 up to 1280, 16-byte aligned with a row stride that is a multiple of 8, and the plan of tome_plan."""
    nimg, H, W, sy, sx, r = (int(v) for v in (nimg, H, W, sy, sx, r))
    if min(nimg, H, W, sy, sx) < 1 or sy > H or sx > W:
        _fail(fn, "nimg, H, W, sy, sx", f"= {nimg}, {H}, {W}, {sy}, {sx}: expected positive sizes and cells inside the "
                                        f"image")
    N = H * W
    Ns = N - (H // sy) * (W // sx)
    if not 0 <= r <= Ns:
        _fail(fn, "r", f"= {r}: outside [0, Ns = {Ns}]")
    _tome_view(fn, x, nimg * (N if rows is None else rows), name)
    if N > TOME_MAX_TOKENS:
        _fail(fn, name, f"{N} tokens per image: at most {TOME_MAX_TOKENS}")
    _block(plan, I32, "plan", fn, shape=(nimg, tome_plan_ints(N)))
    if plan.data_ptr() % 16:
        _fail(fn, "plan", "needs a 16-byte aligned base")
    return N, Ns


def _tome_view(fn, t, rows, name, C=None):
    _view(t, BF16, name, fn, rows=rows)
    c = t.shape[1]
    if c == 0 or c % 64 or c > TOME_MAX_CHANNELS or (C is not None and c != C):
        _fail(fn, name, f"{c} columns: expected {'a multiple of 64' if C is None else C}, at most {TOME_MAX_CHANNELS}")
    if _ld(t) % 8 or t.data_ptr() % 16:
        _fail(fn, name, f"needs a row stride that is a multiple of 8 and a 16-byte aligned base, got stride "
                        f"{t.stride()}")
    return c


def tome_match(x, nimg, H, W, r, plan, *, sy=2, sx=2, seed=None, step_idx=None, layer=0, best=None):
    """The bipartite matching of token merging (vst_tome_match): x [nimg*H*W, C] bf16 view, the metric; writes the plan
    (tome_plan) and returns best, fp32 [nimg, Ns], every source's largest cosine score.  seed (int64 [1]) and step_idx
    (int32 [1]), both or neither: the destination of every cell is drawn from the Philox counters at (seed, step,
    layer, cell), read on the device; neither: the cell's top-left token."""
    fn = "tome_match"
    N, Ns = _tome_operands(fn, x, nimg, H, W, sy, sx, r, plan)
    if (seed is None) != (step_idx is None):
        _fail(fn, "seed, step_idx", "go together")
    if seed is not None:
        _block(seed, torch.int64, "seed", fn, (1,))
        _step_counter(step_idx, fn)
    if not 0 <= int(layer) < 1 << 16:
        _fail(fn, "layer", f"= {layer}: outside [0, 65535]")
    if best is None:
        best = torch.empty((nimg, Ns), dtype=F32, device=x.device)
    _block(best, F32, "best", fn, shape=(nimg, Ns))
    C = x.shape[1]
    Nd = N - Ns
    with _Rec("tome_match", 2.0 * nimg * Ns * Nd * C, 2.0 * nimg * N * C * 2, lambda: "tome_score_kernel",
              (nimg, N, C, r)):
        _lib.call("vst_tome_match", _p(x), _ld(x), int(nimg), int(H), int(W), C, int(sy), int(sx), int(r), _p(seed),
                  _p(step_idx), int(layer), _p(plan), _p(best), _stream())
    return best


def tome_merge(x, nimg, H, W, r, plan, *, sy=2, sx=2, out=None):
    """x [nimg*N, C] -> [nimg*(N - r), C]: every merged row is the mean of its members (vst_tome_merge), in fp32 in
    ascending token order; a row with one member is copied."""
    fn = "tome_merge"
    N, _ = _tome_operands(fn, x, nimg, H, W, sy, sx, r, plan)
    C = x.shape[1]
    out = _new(out, (nimg * (N - r), C), x, "out", fn)
    _tome_view(fn, out, nimg * (N - r), "out", C)
    with _Rec("tome_merge", 1.0 * nimg * N * C, 2.0 * nimg * (2 * N - r) * C, lambda: "tome_merge_kernel",
              (nimg, N, C, r)):
        _lib.call("vst_tome_merge", _p(x), _ld(x), _p(plan), int(nimg), int(H), int(W), C, int(sy), int(sx), int(r),
                  _p(out), _ld(out), _stream())
    return out


def tome_unmerge_add(o, nimg, N, r, plan, *, residual=None, out=None):
    """o [nimg*(N - r), C] -> [nimg*N, C]: out[p] = residual[p] + o[slot[p]] (vst_tome_unmerge_add), or o[slot[p]] bit
    for bit without a residual; out may be the residual."""
    fn = "tome_unmerge_add"
    nimg, N, r = int(nimg), int(N), int(r)
    if nimg < 1 or N < 1 or not 0 <= r < N or N > TOME_MAX_TOKENS:
        _fail(fn, "nimg, N, r", f"= {nimg}, {N}, {r}: expected positive sizes, N <= {TOME_MAX_TOKENS} and 0 <= r < N")
    C = _tome_view(fn, o, nimg * (N - r), "o")
    _block(plan, I32, "plan", fn, shape=(nimg, tome_plan_ints(N)))
    if plan.data_ptr() % 16:
        _fail(fn, "plan", "needs a 16-byte aligned base")
    if residual is not None:
        _tome_view(fn, residual, nimg * N, "residual", C)
    out = _new(out, (nimg * N, C), o, "out", fn)
    _tome_view(fn, out, nimg * N, "out", C)
    with _Rec("tome_unmerge_add", 1.0 * nimg * N * C, 2.0 * nimg * N * C * (2 if residual is None else 3),
              lambda: "tome_unmerge_kernel", (nimg, N, C, r)):
        _lib.call("vst_tome_unmerge_add", _p(o), _ld(o), _p(plan), nimg, N, r, C, _p(residual),
                  0 if residual is None else _ld(residual), _p(out), _ld(out), _stream())
    return out


# ---- ceiling probes (bench.py: measured peaks next to the vendor figures) ----
def probe_mfma_tflops(device, grid=1024, iters=20000, reps=3):
    """Best-of-`reps` bf16 MFMA rate of vst_probe_mfma (16 independent 16x16x32 chains per wave)."""
    sink = torch.empty(grid, dtype=F32, device=device)
    flops = float(grid) * 8 * iters * 16 * 16384
    best = 0.0
    for _ in range(reps + 1):  # first launch warms the clocks
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _lib.call("vst_probe_mfma", grid, iters, sink.data_ptr(), _stream())
        e.record()
        e.synchronize()
        best = max(best, flops / (s.elapsed_time(e) * 1e-3) / 1e12)
    return best


def probe_hbm_read_gbs(device, nbytes=4 << 30, grid=4096, reps=3):
    """Best-of-`reps` streaming read rate of vst_probe_hbm_read over an `nbytes` buffer (>> the 256 MB
    Infinity Cache, so it is HBM)."""
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    sink = torch.empty(grid, dtype=I32, device=device)
    best = 0.0
    for _ in range(reps + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _lib.call("vst_probe_hbm_read", buf.data_ptr(), nbytes, grid, sink.data_ptr(), _stream())
        e.record()
        e.synchronize()
        best = max(best, nbytes / (s.elapsed_time(e) * 1e-3) / 1e9)
    del buf
    return best


# ---- SDXL VAE (AutoencoderKL) pieces (vae.py) ----
def conv3x3_down_pad0(x: torch.Tensor, nimg: int, H: int, W: int, w: torch.Tensor, bias: torch.Tensor | None,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """diffusers Downsample2D(padding=0): F.pad(x, (0,1,0,1)) + 3x3 stride-2 conv, NHWC.  Returns
    [nimg*((H-2)//2+1)*((W-2)//2+1), Cout]."""
    fn = "conv3x3_down_pad0"
    C = _conv_in(x, nimg * H * W, "x", fn)
    _view(w, BF16, "w", fn)
    Cout = w.shape[0]
    if w.shape[1] != 9 * C or C % 64:
        raise _lib.VstError("conv3x3_down_pad0: x [nimg*H*W, C] contiguous, C % 64 == 0, w [Cout, 9C]")
    OH, OW = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    M = nimg * OH * OW
    out = _new(out, (M, Cout), x, "out", fn)
    if bias is not None:
        _vec(bias, Cout, "bias", fn)
    with _Rec("conv3x3", 2.0 * M * Cout * 9 * C, 2.0 * (nimg * H * W * C + Cout * 9 * C + M * Cout),
              lambda: gemm_kernel_name(M, Cout, 9 * C, 2), (M, Cout, 9 * C)):
        ws = _workspace(x.device)
        _lib.call("vst_conv3x3_down_pad0", _p(x), C, nimg, H, W, _p(w), Cout, _p(bias), _p(out), _ld(out), _p(ws),
                  _WS_BYTES, _stream())
    return out


def gemm_f32out(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [M, N] = a[M, K] @ w[N, K]^T without rounding the accumulator."""
    _view(a, BF16, "a", "gemm_f32out")
    _view(w, BF16, "w", "gemm_f32out")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise _lib.VstError(f"gemm_f32out: a {tuple(a.shape)} vs w {tuple(w.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=F32, device=a.device)
    _block(out, F32, "out", "gemm_f32out", (M, N))
    with _Rec("gemm_f32out", 2.0 * M * N * K, 2.0 * (M * K + N * K) + 4.0 * M * N,
              lambda: gemm_kernel_name(M, N, K, 0), (M, N, K)):
        _lib.call("vst_gemm_f32out", _p(a), _ld(a), _p(w), _ld(w), M, N, K, _p(out), _stream())
    return out


def softmax_rows(s: torch.Tensor, scale: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 softmax(scale * s) over the last dim of an fp32 [rows, n] matrix."""
    _view(s, F32, "s", "softmax_rows")
    rows, n = s.shape
    out = _new(out, (rows, n), s, "out", "softmax_rows")
    with _Rec("softmax", 0.0, 4.0 * rows * n + 2.0 * rows * n):
        _lib.call("vst_softmax_rows", _p(s), _ld(s), rows, n, float(scale), _p(out), _ld(out), _stream())
    return out


def _padded_width(ldd, C, fn):
    ldd = C if ldd is None else int(ldd)
    if ldd < C:
        raise _lib.VstError(f"{fn}: ldd {ldd} < C {C}")
    return ldd


def nchw_to_nhwc(x: torch.Tensor, mul: float = 1.0, ldd: int | None = None) -> torch.Tensor:
    """fp32 (n, C, H, W) -> bf16 [n*H*W, ldd] (channels >= C zero)."""
    _block(x, F32, "x", "nchw_to_nhwc")
    if x.dim() != 4:
        raise _lib.VstError("nchw_to_nhwc: x must be a contiguous fp32 (n, C, H, W) device tensor")
    n, C, H, W = x.shape
    ldd = _padded_width(ldd or None, C, "nchw_to_nhwc")
    out = torch.empty((n * H * W, ldd), dtype=BF16, device=x.device)
    _lib.call("vst_nchw_to_nhwc", _p(x), n, C, H * W, float(mul), _p(out), ldd, _stream())
    return out


def _nhwc_in(x, n, C, H, W, fn, name="x"):
    """bf16 rows [n*H*W, >= C] with a row stride >= C."""
    _view(x, BF16, name, fn, rows=n * H * W, min_cols=C)
    if _ld(x) < C:
        _fail(fn, name, f"row stride {_ld(x)} < C = {C}")


def nhwc_to_nchw(x: torch.Tensor, n: int, C: int, H: int, W: int) -> torch.Tensor:
    """bf16 [n*H*W, >=C] -> fp32 (n, C, H, W)."""
    _nhwc_in(x, n, C, H, W, "nhwc_to_nchw")
    out = torch.empty((n, C, H, W), dtype=F32, device=x.device)
    _lib.call("vst_nhwc_to_nchw", _p(x), _ld(x), n, C, H * W, _p(out), _stream())
    return out


def frames_to_u8(x: torch.Tensor, n: int, C: int, H: int, W: int) -> torch.Tensor:
    """bf16 [n*H*W, >=C] decoder output -> uint8 (n, H, W, C) frames (inference_animatediff.py:141-143)."""
    _nhwc_in(x, n, C, H, W, "frames_to_u8")
    out = torch.empty((n, H, W, C), dtype=torch.uint8, device=x.device)
    _lib.call("vst_frames_to_u8", _p(x), _ld(x), n, C, H * W, _p(out), _stream())
    return out


def u8_to_frames(x: torch.Tensor, ldd: int | None = None) -> torch.Tensor:
    """uint8 (n, H, W, C) frames -> bf16 [n*H*W, ldd] rows in [-1, 1] (channels >= C zero): the encoder's input,
    (v / 255 - 0.5) / 0.5 as video_dataset.py:117-118 normalises, rounded to bf16."""
    _block(x, torch.uint8, "x", "u8_to_frames")
    if x.dim() != 4 or x.numel() == 0:
        raise _lib.VstError(f"u8_to_frames: x must be a contiguous uint8 (n, H, W, C) tensor, got {tuple(x.shape)}")
    n, H, W, C = x.shape
    ldd = _padded_width(ldd, C, "u8_to_frames")
    out = torch.empty((n * H * W, ldd), dtype=BF16, device=x.device)
    _lib.call("vst_u8_to_frames", _p(x), n, C, H * W, _p(out), ldd, _stream())
    return out


def vae_sample(moments: torch.Tensor, n: int, H: int, W: int, eps: torch.Tensor | None, mul: float) -> torch.Tensor:
    """moments bf16 [n*H*W, >=8] -> fp32 (n, 4, H, W) = (mean + exp(logvar/2) * eps) * mul (eps None: mean * mul)."""
    _nhwc_in(moments, n, 8, H, W, "vae_sample", "moments")
    if eps is not None:
        _block(eps, F32, "eps", "vae_sample", (n, 4, H, W))
    out = torch.empty((n, 4, H, W), dtype=F32, device=moments.device)
    _lib.call("vst_vae_sample", _p(moments), _ld(moments), n, H * W, _p(eps), float(mul), _p(out), _stream())
    return out
