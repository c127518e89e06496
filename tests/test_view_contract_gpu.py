"""The view contract of the C ABI (include/vst.h): every kernel run on strided views inside guard bands.

The other GPU tests hand the kernels fresh contiguous tensors and read only the output.  Here every case runs twice:
once on plain contiguous operands and once on views cut out of larger buffers, and four things are asserted.

  1. Outputs are sentinel-prefilled arenas (bf16 0x7FA5, fp32 0x7FC0A5A5, written and compared as integers).  After
     the launch every element outside the view still holds the sentinel: no write leaves [rows) x [cols).
  2. No element of the view holds the sentinel or a non-finite value: every element was written, and nothing leaked
     in from the operands' padding, which is NaN everywhere around the data.
  3. The view's bits equal the contiguous call's bits (strides change no arithmetic; tile policies are shape-only).
     "Contiguous" is as dense as the ABI takes the operand: every row stride must be a multiple of 8 elements, so
     a 332-wide matrix runs with ld = 336 there, against ld = 352 and a column offset in the arena.
  4. The values agree with an fp32 torch reference written here from the operands, at the bars the existing test of
     the same wrapper uses (test_kernels_gpu.check: rel-L2 5e-3 / rel-max 1e-2 for forward kernels; rel-L2 2e-2
     for the backward kernels, test_training_gpu; 1e-6 for colsum).

An arena has 8 guard rows above, 320 below (one tile more than the tallest, 256-row, tile) and 8 guard columns on each
side, so a whole unmasked tile would still land in memory the test owns and be reported by (1).  The contiguous
run's outputs have the same guard rows.  Operands that the ABI wants contiguous (conv inputs and weights, fp32
vectors) are slices of a NaN-filled 1-D buffer with at least one row / image of NaN on each side.

Shapes are the smallest with a full tile plus a tail in M and N, a K tail and two k-tiles (M=300, N=332, K=200 for
the projections).  Shapes moved from the first choice because an entry point's policy does not take them:
  * the persistent 8-phase grid needs two rounds of tiles (>= 2 x CUs = 512 tiles on the MI355X), so the two
    persistent cases use M = 4680 (36 x 128 + 72; 37 x 14 = 518 tiles of 128x320) and M = 5448 (21 x 256 + 72;
    22 x 24 = 528 GEGLU tiles of 256x256) instead of M = 2632;
  * 3x3 convs reach the 8-phase kernel only from half a wave of 256x256 tiles on (no tile code forces it), so the
    8-phase conv cases use two 91x91 images (M = 16562 = 129 x 128 + 50) instead of 9x9;
  * the frame-axis attention takes head sizes 8 .. 160, so (nclip, F, HW, C) = (1, 16, 8, 80) runs as two heads of
    40, not eight of 10.
Outputs a wrapper allocates itself (dx / dgamma / dbeta of the norm backward kernels, the outputs of zero_insert and
sumpool2x2) get checks 3 and 4 only.
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = {BF16: (torch.int16, 0x7FA5), F32: (torch.int32, 0x7FC0A5A5)}
GUARD_TOP, GUARD_BOTTOM, GUARD_COL = 8, 320, 8
FWD, BWD = (5e-3, 1e-2), (2e-2, None)


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


# ---------------------------------------------------------------- harness
def _fill(t, fill):
    if fill == "sentinel":
        itype, bits = SENTINEL[t.dtype]
        t.view(itype).fill_(bits)
    else:
        t.fill_(fill)
    return t


def arena(rows, cols, dtype, fill, device):
    """(view, arena): the interior [8:8+rows, 8:8+cols] of one (8 + rows + 320) x ld tensor filled with `fill`;
    ld = 8 + cols + 8 rounded up to a multiple of 8 elements (so ld != cols and the interior is 16-byte aligned)."""
    ld = (GUARD_COL + cols + GUARD_COL + 7) // 8 * 8
    a = _fill(torch.empty((GUARD_TOP + rows + GUARD_BOTTOM, ld), dtype=dtype, device=device), fill)
    return a[GUARD_TOP:GUARD_TOP + rows, GUARD_COL:GUARD_COL + cols], a


def dense(rows, cols, dtype, fill, device, flat=False):
    """(view, buffer): [rows, cols] as densely as the ABI takes it, with the arena's guard rows: contiguous, or for a
    width that is no multiple of 8 elements a row stride rounded up to one (every ld must be a multiple of 8, so
    N = 332 has no contiguous form; the up to 7 pad columns are guard like the rows)."""
    ld = cols if flat else (cols + 7) // 8 * 8
    a = _fill(torch.empty((GUARD_TOP + rows + GUARD_BOTTOM, ld), dtype=dtype, device=device), fill)
    return a[GUARD_TOP:GUARD_TOP + rows, :cols], a


def contig_in(x, device, guard):
    """x as a contiguous slice of a NaN-filled 1-D buffer, `guard` elements (rounded up to 32 bytes) of NaN on each
    side."""
    pad = (max(int(guard), 8) + 7) // 8 * 8
    n = x.numel()
    buf = torch.full((pad + n + pad,), float("nan"), dtype=x.dtype, device=device)
    buf[pad:pad + n].copy_(x.reshape(-1))
    v = buf[pad:pad + n].view(x.shape)
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def _bbox(mask, r0, c0):
    idx = mask.nonzero()
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    return f"rows [{lo[0] - r0}, {hi[0] - r0}] x cols [{lo[1] - c0}, {hi[1] - c0}] relative to the view ({len(idx)} elements)"


def verify_out(name, full, r0, c0, rows, cols, untouched=False):
    itype, bits = SENTINEL[full.dtype]
    same = full.view(itype) == bits
    changed = ~same
    if not untouched:
        changed[r0:r0 + rows, c0:c0 + cols] = False
    assert not changed.any(), f"{name}: guard band written at {_bbox(changed, r0, c0)}"
    if untouched:
        return
    inner = full[r0:r0 + rows, c0:c0 + cols]
    bad = same[r0:r0 + rows, c0:c0 + cols] | ~torch.isfinite(inner.float())
    assert not bad.any(), f"{name}: view elements unwritten or non-finite at {_bbox(bad, 0, 0)}"


def check(out, ref, tol, name):
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), name
    err = out - ref
    l2 = (err.norm() / ref.norm().clamp_min(1e-12)).item()
    mx = (err.abs().max() / ref.abs().max().clamp_min(1e-12)).item()
    print(f"[view] {name}: rel_l2={l2:.3e} rel_max={mx:.3e}")
    assert l2 <= tol[0] and (tol[1] is None or mx <= tol[1]), f"{name}: rel_l2={l2:.3e} rel_max={mx:.3e} (bar {tol})"


def _bits(t):
    t = t.contiguous()
    return t.view(SENTINEL[t.dtype][0])


class Spec:
    """One wrapper call.  ins: name -> (CPU tensor or None, "view" | "contig"); fused: buffer name -> the ins that are
    column views of it; outs: name -> (rows, cols, dtype, "view" | "flat" | "vec"); run(K, t) launches on the device
    tensors t (and may return more outputs by name); ref(i) -> name -> fp32 reference from the CPU operands i."""

    def __init__(self, ins, outs, run, ref, *, fused=None, guard=None, tol=None, default_tol=FWD, policy=None,
                 kernel=None):
        self.ins, self.outs, self.run, self.ref = ins, outs, run, ref
        self.fused, self.guard, self.tol, self.default_tol = fused or {}, guard or {}, tol or {}, default_tol
        self.policy, self.kernel = policy or {}, kernel


@contextlib.contextmanager
def policy(K, tile=0, splits=0, bn=None, persist=None, p8conv=None, sa_self=None):
    with contextlib.ExitStack() as st:
        if bn is not None:
            st.enter_context(K.p8_tile_width(bn))
        if persist is not None:
            st.enter_context(K.p8_persist(persist))
        if p8conv is not None:
            st.enter_context(K.p8_conv(p8conv))
        if sa_self is not None:
            st.enter_context(K.sa_self(sa_self))
        K.GEMM_POLICY.update(tile=tile, splits=splits)
        try:
            yield
        finally:
            K.GEMM_POLICY.update(tile=0, splits=0)


def materialize(spec, dev, strided):
    t, arenas = {}, {}
    in_fused = {n for names in spec.fused.values() for n in names}
    nan = float("nan")
    for name, (x, kind) in spec.ins.items():
        if x is None:
            t[name] = None
        elif name in in_fused:
            continue
        elif kind == "contig":
            t[name] = contig_in(x, dev, spec.guard.get(name, x.shape[-1]))
        elif strided:
            v, _ = arena(x.shape[0], x.shape[1], x.dtype, nan, dev)
            v.copy_(x)
            t[name] = v
        else:
            t[name], _ = dense(x.shape[0], x.shape[1], x.dtype, nan, dev)
            t[name].copy_(x)
    for names in spec.fused.values():
        xs = [spec.ins[n][0] for n in names]
        if strided:
            v, _ = arena(xs[0].shape[0], sum(x.shape[1] for x in xs), xs[0].dtype, nan, dev)
            v.copy_(torch.cat(xs, 1))
            c = 0
            for n, x in zip(names, xs):
                t[n] = v[:, c:c + x.shape[1]]
                c += x.shape[1]
        else:
            for n, x in zip(names, xs):
                t[n], _ = dense(x.shape[0], x.shape[1], x.dtype, nan, dev)
                t[n].copy_(x)
    for name, (rows, cols, dtype, kind) in spec.outs.items():
        if strided and kind in ("view", "vec"):
            v, full = arena(rows, cols, dtype, "sentinel", dev)
            off = (GUARD_TOP, GUARD_COL)
        else:
            v, full = dense(rows, cols, dtype, "sentinel", dev, flat=kind != "view")
            off = (GUARD_TOP, 0)
        t[name] = v[0] if kind == "vec" else v
        arenas[name] = (full, off[0], off[1], rows, cols)
    return t, arenas


def run_case(K, dev, spec):
    cpu = {n: x for n, (x, _) in spec.ins.items()}
    refs = spec.ref(cpu)
    res = {}
    with policy(K, **spec.policy):
        if spec.kernel is not None:
            args, want = spec.kernel
            name = K.gemm_kernel_name(*args)
            assert want in name, (name, want)
        for strided in (False, True):
            t, arenas = materialize(spec, dev, strided)
            extra = spec.run(K, t)
            extra = extra if isinstance(extra, dict) else {}
            torch.cuda.synchronize()
            res[strided] = (t, arenas, extra)
    for strided in (False, True):
        t, arenas, extra = res[strided]
        tag = "strided" if strided else "contiguous"
        for name, (full, r0, c0, rows, cols) in arenas.items():
            verify_out(f"{name} ({tag})", full, r0, c0, rows, cols)
        for name, v in extra.items():
            assert torch.isfinite(v.float()).all(), f"{name} ({tag}): non-finite"
    (tc, _, ec), (ts, _, es) = res[False], res[True]
    for name in list(spec.outs) + list(es):
        a = ts[name] if name in spec.outs else es[name]
        b = tc[name] if name in spec.outs else ec[name]
        diff = _bits(a) != _bits(b)
        assert not diff.any(), (f"{name}: strided and contiguous bits differ in {int(diff.sum())} elements, max |d| = "
                                f"{(a.float() - b.float()).abs().max().item():.3e}")
        assert name in refs, f"no reference for {name}"
        check(a.reshape(refs[name].shape), refs[name], spec.tol.get(name, spec.default_tol), name)


# ---------------------------------------------------------------- operand helpers
def gen(*key):
    s = 0
    for k in key:
        s = s * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))
    return torch.Generator().manual_seed(s % (2 ** 31))


def rnd(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def bf(x):
    return x.to(BF16).float()


def to_nhwc(x):  # (N,C,H,W) -> [N*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def wflat(w):  # (Cout,Cin,3,3) -> [Cout, 9*Cin] (ky,kx,ci)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def geglu_ref(y):
    N = y.shape[1]
    idx = torch.arange(N).view(-1, 64)
    return y[:, idx[:, :32].reshape(-1)] * F.gelu(y[:, idx[:, 32:].reshape(-1)])


# ---------------------------------------------------------------- adapters
def linear_spec(M, N, K1, K2=0, epi="bias", div=64, **kw):
    g = gen("linear", M, N, K1, K2, epi)
    Kt, geglu = K1 + K2, epi == "geglu"
    nout = N // 2 if geglu else N
    ins = {"x": (rnd(M, K1, g=g), "view"), "x2": (rnd(M, K2, g=g) if K2 else None, "view"),
           "w": (rnd(N, Kt, scale=Kt ** -0.5, g=g), "view"),
           "bias": (None if epi == "none" else torch.randn(N, generator=g), "contig"),
           "residual": (rnd(M, nout, g=g) if epi == "res" else None, "view"),
           "row_bias": (torch.randn((M + div - 1) // div, N, generator=g) if epi == "rowbias" else None, "view")}

    def run(K, t):
        K.linear(t["x"], t["w"], t["bias"], x2=t["x2"], residual=t["residual"], row_bias=t["row_bias"],
                 row_bias_div=div, out=t["out"], geglu=geglu, act="gelu" if epi == "gelu" else None)

    def ref(i):
        xx = i["x"].float() if K2 == 0 else torch.cat([i["x"], i["x2"]], 1).float()
        y = xx @ i["w"].float().t() + (0 if i["bias"] is None else i["bias"])
        if geglu:
            y = geglu_ref(y)
        elif epi == "gelu":
            y = F.gelu(y)
        elif epi == "res":
            y = bf(y) + i["residual"].float()
        elif epi == "rowbias":
            y = bf(y) + i["row_bias"].repeat_interleave(div, 0)[:M]
        return {"out": y}

    return Spec(ins, {"out": (M, nout, BF16, "view")}, run, ref, fused={"xx": ["x", "x2"]} if K2 else None, **kw)


def lora_spec(M, Kd, N, P, gn, gr, bn):
    g = gen("lora", M, Kd, N, P)
    A = torch.zeros(P, Kd)
    A[:gr] = torch.randn(gr, Kd, generator=g) * Kd ** -0.5
    W = torch.zeros(N, Kd + P)
    W[:, :Kd] = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    W[:, Kd:Kd + gr] = torch.randn(N, gr, generator=g) * gr ** -0.5
    ins = {"x": (rnd(M, Kd, g=g), "view"), "a": (A.to(BF16), "view"), "w": (W.to(BF16), "view"),
           "bias": (torch.randn(N, generator=g) * 0.1, "contig"), "residual": (rnd(M, N, g=g), "view")}

    def run(K, t):
        assert K.gemm_lora_tile(M, N, Kd, P, gn, gr) == bn
        K.linear_lora(t["x"], t["w"], t["a"], gn, gr, t["bias"], residual=t["residual"], out=t["out"])

    def ref(i):
        x, w = i["x"].float(), i["w"].float()
        u = bf(x @ i["a"].float().t())
        return {"out": bf(x @ w[:, :Kd].t() + u @ w[:, Kd:].t() + i["bias"]) + i["residual"].float()}

    return Spec(ins, {"out": (M, N, BF16, "view")}, run, ref, policy=dict(bn=bn))


def sdpa_ref(q, k, v, nb, heads, Nq, Nk, kv_div, scale=0.125):
    """(o [nb*Nq, C], log2-domain logsumexp [nb*heads*Nq]) in fp32; text batch of q batch b is b // kv_div."""
    C = heads * 64
    qh = q.float().view(nb, Nq, heads, 64).transpose(1, 2)
    idx = torch.arange(nb) // kv_div
    kh = k.float().reshape(-1, Nk, heads, 64).transpose(1, 2)[idx]
    vh = v.float().reshape(-1, Nk, heads, 64).transpose(1, 2)[idx]
    s = qh @ kh.transpose(-1, -2) * scale
    o = torch.softmax(s, -1) @ vh
    return o.transpose(1, 2).reshape(nb * Nq, C), (torch.logsumexp(s, -1) / math.log(2.0)).reshape(-1)


def xattn_spec(frames, Nq, N, Kd, Nk, kv_div, lora):
    g = gen("xattn", frames, Nq, N, Kd, lora)
    M, heads, P = frames * Nq, N // 64, 32 if lora else 0
    nb = (frames + kv_div - 1) // kv_div
    W = torch.zeros(N, Kd + P)
    W[:, :Kd] = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    A = None
    if lora:
        W[:, Kd:Kd + 16] = torch.randn(N, 16, generator=g) * 0.25
        A = torch.zeros(P, Kd)
        A[:16] = torch.randn(16, Kd, generator=g) * Kd ** -0.5
        A = A.to(BF16)
    ins = {"x": (rnd(M, Kd, g=g), "view"), "w": (W.to(BF16), "view"), "a": (A, "view"),
           "bias": (torch.randn(N, generator=g) * 0.1, "contig"),
           "k": (rnd(nb * Nk, N, scale=2.0, g=g), "view"), "v": (rnd(nb * Nk, N, scale=2.0, g=g), "view")}

    def run(K, t):
        K.linear_cross_attention(t["x"], t["w"], t["a"], N, 16, t["bias"], t["k"], t["v"], Nq=Nq, Nk=Nk,
                                 kv_div=kv_div, scale=0.125, out=t["out"])

    def ref(i):
        x, w = i["x"].float(), i["w"].float()
        q = x @ w[:, :Kd].t() + i["bias"]
        if lora:
            q = q + bf(x @ i["a"].float().t()) @ w[:, Kd:].t()
        return {"out": sdpa_ref(bf(q), i["k"], i["v"], frames, heads, Nq, Nk, kv_div)[0]}

    return Spec(ins, {"out": (M, N, BF16, "view")}, run, ref, fused={"kv": ["k", "v"]})


def seq_attn_ref(q, k, v, nclip, Fr, HW, heads, d):
    def seq(t):  # rows (b*F+f)*HW+p -> (b*HW+p, heads, F, d)
        return t.float().view(nclip, Fr, HW, heads, d).permute(0, 2, 3, 1, 4).reshape(nclip * HW, heads, Fr, d)

    o = torch.softmax(seq(q) @ seq(k).transpose(-1, -2) / math.sqrt(d), -1) @ seq(v)
    return o.view(nclip, HW, heads, Fr, d).permute(0, 3, 1, 2, 4).reshape(nclip * Fr * HW, heads * d)


def tattn_fused_spec(nclip, Fr, HW, Kd, heads, d):
    from video_style_transfer_amd import kernels
    g = gen("tattn_fused", nclip, HW, heads, d)
    C, M = heads * d, nclip * Fr * HW
    w = rnd(3 * C, Kd, scale=Kd ** -0.5, g=g)
    b = torch.randn(3 * C, generator=g) * 0.1
    w_t, b_t = kernels.temporal_qkv_layout(w, b, heads, d)  # (pure torch: laid out on the CPU)
    ins = {"x": (rnd(M, Kd, g=g), "view"), "w_t": (w_t, "view"), "b_t": (b_t, "contig")}

    def run(K, t):
        K.linear_temporal_attention(t["x"], t["w_t"], t["b_t"], nclip=nclip, F=Fr, HW=HW, heads=heads, head_dim=d,
                                    scale=d ** -0.5, out=t["out"])

    def ref(i):
        qkv = bf(i["x"].float() @ w.float().t() + b)
        return {"out": seq_attn_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], nclip, Fr, HW, heads, d)}

    return Spec(ins, {"out": (M, C, BF16, "view")}, run, ref)


def conv_spec(n, H, W, C1, C2, Co, stride=1, up=False, **kw):
    g = gen("conv", n, H, C1, C2, Co, stride, int(up))
    Ct = C1 + C2
    x1 = rnd(n, C1, H, W, g=g)
    x2 = rnd(n, C2, H, W, g=g) if C2 else None
    w = rnd(Co, Ct, 3, 3, scale=(9 * Ct) ** -0.5, g=g)
    OH, OW = (2 * H, 2 * W) if up else ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    M = n * OH * OW
    r = rnd(n, Co, OH, OW, g=g)
    ins = {"x1": (to_nhwc(x1), "contig"), "x2": (None if x2 is None else to_nhwc(x2), "contig"),
           "w": (wflat(w), "contig"), "bias": (torch.randn(Co, generator=g) * 0.1, "contig"),
           "row_bias": (torch.randn(n, Co, generator=g), "view"), "residual": (to_nhwc(r), "view")}
    guard = {"x1": H * W * C1, "x2": H * W * C2}  # one image of NaN before and after: a halo read past an end shows

    def run(K, t):
        K.conv3x3(t["x1"], n, H, W, t["w"], t["bias"], x2=t["x2"], stride=stride, upsample=up,
                  row_bias=t["row_bias"], row_bias_div=OH * OW, residual=t["residual"], out=t["out"])

    def ref(i):
        xx = x1.float() if x2 is None else torch.cat([x1, x2], 1).float()
        if up:
            xx = F.interpolate(xx, scale_factor=2.0, mode="nearest")
        y = bf(F.conv2d(xx, w.float(), i["bias"], stride=stride, padding=1))
        return {"out": to_nhwc(y + i["row_bias"][:, :, None, None] + r.float())}

    return Spec(ins, {"out": (M, Co, BF16, "view")}, run, ref, guard=guard, **kw)


def conv_down_pad0_spec(n, H, W, C, Co):
    g = gen("pad0", n, H, C, Co)
    x = rnd(n, C, H, W, g=g)
    w = rnd(Co, C, 3, 3, scale=(9 * C) ** -0.5, g=g)
    OH, OW = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    ins = {"x": (to_nhwc(x), "contig"), "w": (wflat(w), "contig"), "bias": (torch.randn(Co, generator=g) * 0.1, "contig")}

    def run(K, t):
        K.conv3x3_down_pad0(t["x"], n, H, W, t["w"], t["bias"], out=t["out"])

    def ref(i):
        return {"out": to_nhwc(F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), i["bias"], stride=2))}

    return Spec(ins, {"out": (n * OH * OW, Co, BF16, "view")}, run, ref, guard={"x": H * W * C})


def spatial_spec(nb, heads, Nq, Nk, kv_div, self_on):
    g = gen("spatial", nb, heads, Nq, Nk, kv_div)
    C, nkv = heads * 64, nb // kv_div
    ins = {"q": (rnd(nb * Nq, C, g=g), "view"), "k": (rnd(nkv * Nk, C, g=g), "view"),
           "v": (rnd(nkv * Nk, C, g=g), "view")}
    fused = {"qkv": ["q", "k", "v"]} if nb * Nq == nkv * Nk else {"kv": ["k", "v"]}

    def run(K, t):
        K.spatial_attention(t["q"], t["k"], t["v"], nb, heads, Nq, Nk, kv_div, out=t["out"], lse=t["lse"])

    def ref(i):
        o, lse = sdpa_ref(i["q"], i["k"], i["v"], nb, heads, Nq, Nk, kv_div)
        return {"out": o, "lse": lse}

    return Spec(ins, {"out": (nb * Nq, C, BF16, "view"), "lse": (1, nb * heads * Nq, F32, "vec")}, run, ref,
                fused=fused, policy=dict(sa_self=self_on))


def temporal_heads(C):
    """8 heads as the motion modules have, where C / 8 is a head size the kernels take (8 .. 160); C = 80 runs as two
    heads of 40 (ten-wide heads are refused)."""
    return (8, C // 8) if C // 8 in (8, 16, 32, 40, 64, 80, 160) else (C // 40, 40)


def temporal_spec(nclip, Fr, HW, C):
    g = gen("temporal", nclip, Fr, HW, C)
    (heads, d), rows = temporal_heads(C), nclip * Fr * HW
    ins = {n: (rnd(rows, C, g=g), "view") for n in ("q", "k", "v")}

    def run(K, t):
        K.temporal_attention(t["q"], t["k"], t["v"], nclip, Fr, HW, heads, d, out=t["out"])

    def ref(i):
        return {"out": seq_attn_ref(i["q"], i["k"], i["v"], nclip, Fr, HW, heads, d)}

    return Spec(ins, {"out": (rows, C, BF16, "view")}, run, ref, fused={"qkv": ["q", "k", "v"]})


def gn_ref(x, ns, rps, gam, bet, eps, silu):
    C = x.shape[1]
    y = F.group_norm(x.float().view(ns, rps, C).permute(0, 2, 1), 32, gam, bet, eps).permute(0, 2, 1).reshape(-1, C)
    return F.silu(y) if silu else y


def group_norm_spec(rows, C, silu):
    g = gen("gn", rows, C, int(silu))
    ns, rps = 2, rows // 2
    C1 = 32 if C == 64 else 192  # groups of C / 32 channels: 192 | 128 puts a group across the seam
    ins = {"x1": (rnd(rows, C1, g=g) + 0.5, "view"), "x2": (rnd(rows, C - C1, g=g), "view"),
           "gamma": (torch.rand(C, generator=g) + 0.5, "contig"), "beta": (torch.randn(C, generator=g) * 0.1, "contig")}

    def run(K, t):
        K.group_norm(t["x1"], ns, rps, 32, 1e-5, t["gamma"], t["beta"], silu=silu, x2=t["x2"], out=t["out"])

    def ref(i):
        return {"out": gn_ref(torch.cat([i["x1"], i["x2"]], 1), ns, rps, i["gamma"], i["beta"], 1e-5, silu)}

    return Spec(ins, {"out": (rows, C, BF16, "view")}, run, ref)


def gn_partials_spec(rows, C):
    g = gen("gnp", rows, C)
    nclips, fl, rpf = (2, 3, 50) if rows == 300 else (1, 2, 35)
    ins = {"x": (rnd(rows, C, g=g) + 0.3, "view"), "gamma": (torch.rand(C, generator=g) + 0.5, "contig"),
           "beta": (torch.randn(C, generator=g) * 0.1, "contig")}

    def run(K, t):
        part = K.group_norm_frame_partials(t["x"], nclips * fl, rpf, 32)
        K.group_norm_apply_partials(t["x"], nclips, fl, rpf, 32, 1e-6, t["gamma"], t["beta"], part, 1, silu=True,
                                    out=t["out"])

    def ref(i):
        return {"out": gn_ref(i["x"], nclips, fl * rpf, i["gamma"], i["beta"], 1e-6, True)}

    return Spec(ins, {"out": (rows, C, BF16, "view")}, run, ref)


def layer_norm_spec(rows, C, lora):
    g = gen("ln", rows, C, int(lora))
    HW, Fr, R = 4, 8, 16
    ins = {"x": (rnd(rows, C, g=g) + 0.3, "view"), "gamma": (torch.rand(C, generator=g) + 0.5, "contig"),
           "beta": (torch.randn(C, generator=g) * 0.1, "contig")}
    if lora:
        ins["A"] = (rnd(R, C, scale=C ** -0.5, g=g), "contig")
    else:
        ins["pe"] = (torch.randn(32, C, generator=g), "contig")

    def run(K, t):
        if lora:
            K.layer_norm_lora(t["x"], t["gamma"], t["beta"], 1e-5, t["A"], out=t["out"], u=t["u"])
        else:
            K.layer_norm(t["x"], t["gamma"], t["beta"], 1e-5, pe=t["pe"], pe_div=HW, pe_mod=Fr, out=t["out"])

    def ref(i):
        y = F.layer_norm(i["x"].float(), (C,), i["gamma"], i["beta"], 1e-5)
        if lora:
            return {"out": y, "u": bf(y) @ i["A"].float().t()}
        return {"out": y + i["pe"][(torch.arange(rows) // HW) % Fr]}

    outs = {"out": (rows, C, BF16, "view")}
    if lora:
        outs["u"] = (rows, R, BF16, "view")
    return Spec(ins, outs, run, ref)


def rowop_spec(op, rows, C):
    g = gen(op, rows, C)
    x = rnd(rows, C, g=g)
    if op == "add_row_table":
        ins = {"x": (x, "view"), "table": (torch.randn(32, C, generator=g), "contig")}
        run = lambda K, t: K.add_row_table(t["x"], t["table"], div=5, mod=7, out=t["out"])
        ref = lambda i: {"out": i["x"].float() + i["table"][(torch.arange(rows) // 5) % 7]}
        outs = {"out": (rows, C, BF16, "view")}
    elif op == "permute_rows":
        dims, perm = ((3, 4, 5, 5), (1, 2, 0, 3)) if rows == 300 else ((2, 5, 7, 1), (2, 0, 1, 3))
        ins = {"x": (x, "contig")}
        run = lambda K, t: K.permute_rows(t["x"], dims, perm, out=t["out"])
        ref = lambda i: {"out": i["x"].float().view(*dims, C).permute(*perm, 4).reshape(rows, C)}
        outs = {"out": (rows, C, BF16, "flat")}
    elif op == "transpose":
        ins = {"x": (x, "view")}
        run = lambda K, t: K.transpose(t["x"], out=t["out"])
        ref = lambda i: {"out": i["x"].float().t()}
        outs = {"out": (C, rows, BF16, "view")}
    elif op == "copy2d":
        ins = {"x": (x, "view")}
        run = lambda K, t: K.copy2d(t["x"], t["out"])
        ref = lambda i: {"out": i["x"].float()}
        outs = {"out": (rows, C, BF16, "view")}
    elif op == "softmax_rows":
        ins = {"x": (torch.randn(rows, C, generator=g) * 3.0, "view")}
        run = lambda K, t: K.softmax_rows(t["x"], 0.3, out=t["out"])
        ref = lambda i: {"out": torch.softmax(0.3 * i["x"], -1)}
        outs = {"out": (rows, C, BF16, "view")}
    elif op == "gemm_f32out":
        Kd = 200
        ins = {"x": (rnd(rows, Kd, g=g), "view"), "w": (rnd(C, Kd, scale=Kd ** -0.5, g=g), "view")}
        run = lambda K, t: K.gemm_f32out(t["x"], t["w"], out=t["out"])
        ref = lambda i: {"out": i["x"].float() @ i["w"].float().t()}
        outs = {"out": (rows, C, F32, "flat")}
    return Spec(ins, outs, run, ref)


def linear_tn_spec(M, N, Kc):
    g = gen("tn", M, N, Kc)
    ins = {"a": (rnd(M, N, g=g), "view"), "b": (rnd(M, Kc, scale=M ** -0.5, g=g), "view")}

    def run(K, t):
        assert (K._lib.load().vst_gemm_tn_workspace_bytes(M, N, Kc) > 0) == (M > 2048)  # direct / split path
        K.linear_tn(t["a"], t["b"], out=t["out"])

    return Spec(ins, {"out": (N, Kc, BF16, "view")}, run, lambda i: {"out": i["a"].float().t() @ i["b"].float()})


def layer_norm_bwd_spec(rows, C):
    g = gen("lnb", rows, C)
    ins = {"x": (rnd(rows, C, g=g) + 0.3, "view"), "g": (rnd(rows, C, g=g), "view"),
           "gamma": (torch.rand(C, generator=g) + 0.5, "contig")}

    def run(K, t):
        dx, dgamma, dbeta = K.layer_norm_bwd(t["x"], t["g"], t["gamma"], 1e-5)
        return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}

    def ref(i):
        xr, gr, br = i["x"].float().requires_grad_(True), i["gamma"].clone().requires_grad_(True), \
            torch.zeros(C, requires_grad=True)
        F.layer_norm(xr, (C,), gr, br, 1e-5).backward(i["g"].float())
        return {"dx": xr.grad, "dgamma": gr.grad, "dbeta": br.grad}

    return Spec(ins, {}, run, ref, default_tol=BWD)


def group_norm_bwd_spec(rows, C, silu):
    g = gen("gnb", rows, C, int(silu))
    ns, rps = 2, rows // 2
    ins = {"x": (rnd(rows, C, g=g) + 0.5, "view"), "g": (rnd(rows, C, g=g), "view"),
           "gamma": (torch.rand(C, generator=g) + 0.5, "contig"), "beta": (torch.randn(C, generator=g) * 0.1, "contig")}

    def run(K, t):
        dx, dgamma, dbeta = K.group_norm_bwd(t["x"], t["g"], ns, rps, 32, 1e-6, t["gamma"], t["beta"], silu=silu)
        return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}

    def ref(i):
        xr, gr, br = (i[n].float().clone().requires_grad_(True) for n in ("x", "gamma", "beta"))
        gn_ref(xr, ns, rps, gr, br, 1e-6, silu).backward(i["g"].float())
        return {"dx": xr.grad, "dgamma": gr.grad, "dbeta": br.grad}

    return Spec(ins, {}, run, ref, default_tol=BWD)


def geglu_bwd_spec(M, Nh):
    g = gen("geglub", M, Nh)
    ins = {"p": (rnd(M, 2 * Nh, g=g), "view"), "g": (rnd(M, Nh, g=g), "view")}

    def ref(i):
        pr = i["p"].float().requires_grad_(True)
        blk = pr.view(M, Nh // 32, 2, 32)  # [32 hidden | 32 gate] per 64 columns, as the fused GEMM stores p
        (blk[:, :, 0].reshape(M, Nh) * F.gelu(blk[:, :, 1].reshape(M, Nh))).backward(i["g"].float())
        return {"out": pr.grad}

    return Spec(ins, {"out": (M, 2 * Nh, BF16, "view")}, lambda K, t: K.geglu_bwd(t["p"], t["g"], out=t["out"]), ref,
                default_tol=BWD)


def colsum_spec(M, N):
    g = gen("colsum", M, N)
    ins = {"x": (rnd(M, N, g=g), "view")}
    return Spec(ins, {"out": (1, N, F32, "vec")}, lambda K, t: K.colsum(t["x"], out=t["out"]),
                lambda i: {"out": i["x"].double().sum(0).float()}, default_tol=(1e-6, None))


def spatial_bwd_spec(nb, heads, Nq, Nk, kv_div):
    g = gen("sab", nb, heads, Nq, Nk)
    C, nkv = heads * 64, nb // kv_div
    ins = {"q": (rnd(nb * Nq, C, g=g), "view"), "k": (rnd(nkv * Nk, C, g=g), "view"),
           "v": (rnd(nkv * Nk, C, g=g), "view"), "dout": (rnd(nb * Nq, C, g=g), "view")}

    def run(K, t):
        lse = torch.empty(nb * heads * Nq, dtype=F32, device=t["q"].device)
        o = K.spatial_attention(t["q"], t["k"], t["v"], nb, heads, Nq, Nk, kv_div, lse=lse)
        K.spatial_attention_bwd(t["q"], t["k"], t["v"], o, t["dout"], lse, nb, heads, Nq, Nk, kv_div, dq=t["dq"],
                                dkv=t["dkv"])

    def ref(i):
        qr, kr, vr = (i[n].float().requires_grad_(True) for n in ("q", "k", "v"))
        sdpa_ref(qr, kr, vr, nb, heads, Nq, Nk, kv_div)[0].backward(i["dout"].float())
        return {"dq": qr.grad, "dkv": torch.cat([kr.grad, vr.grad], 1)}

    return Spec(ins, {"dq": (nb * Nq, C, BF16, "view"), "dkv": (nkv * Nk, 2 * C, BF16, "view")}, run, ref,
                fused={"kv": ["k", "v"]}, default_tol=BWD)


def temporal_bwd_spec(nclip, Fr, HW, C):
    g = gen("tab", nclip, Fr, HW, C)
    (heads, d), rows = temporal_heads(C), nclip * Fr * HW
    ins = {n: (rnd(rows, C, g=g), "view") for n in ("q", "k", "v", "dout")}

    def run(K, t):
        K.temporal_attention_bwd(t["q"], t["k"], t["v"], t["dout"], nclip, Fr, HW, heads, d, out=t["out"])

    def ref(i):
        qr, kr, vr = (i[n].float().requires_grad_(True) for n in ("q", "k", "v"))
        seq_attn_ref(qr, kr, vr, nclip, Fr, HW, heads, d).backward(i["dout"].float())
        return {"out": torch.cat([qr.grad, kr.grad, vr.grad], 1)}

    return Spec(ins, {"out": (rows, 3 * C, BF16, "view")}, run, ref, fused={"qkv": ["q", "k", "v"]}, default_tol=BWD)


def sampler_dgrad_spec(op, n, h, w, C):
    """zero_insert / sumpool2x2 (h, w: the small grid): x is addressed as one contiguous block, so it is a slice of a
    NaN buffer with one image of NaN on each side; the wrappers allocate their outputs."""
    g = gen(op, n, h, w, C)
    if op == "zero_insert":
        x = rnd(n, h, w, C, g=g)
        run = lambda K, t: {"out": K.zero_insert(t["x"], n, h, w)}

        def ref(i):
            y = torch.zeros(n, 2 * h, 2 * w, C)
            y[:, ::2, ::2] = x.float()
            return {"out": y.reshape(-1, C)}
    else:
        x = rnd(n, 2 * h, 2 * w, C, g=g)
        run = lambda K, t: {"out": K.sumpool2x2(t["x"], n, h, w)}
        ref = lambda i: {"out": x.float().view(n, h, 2, w, 2, C).sum((2, 4)).reshape(-1, C)}
    return Spec({"x": (x.reshape(-1, C), "contig")}, {}, run, ref, guard={"x": x[0].numel()})


# ---------------------------------------------------------------- the matrix
CASES = {}


def case(cid, fn, *a, **kw):
    assert cid not in CASES, cid
    CASES[cid] = (fn, a, kw)


M0, N0, K0 = 300, 332, 200  # 332 = 256 + 76 = 192 + 140; 76 leaves a 4-column chunk; 200 = 3 x 64 + 8
RING_SPLITS = {1: 3, 2: 2, 3: 2, 4: 3, 6: 3, 7: 2}
for _tile in (1, 2, 3, 4, 6, 7, 8, 9):
    _fam = "p8" if _tile >= 8 else "ring"
    for _epi in ("bias", "res", "rowbias", "gelu"):
        case(f"linear-{_fam}-t{_tile}-{_epi}", linear_spec, M0, N0, K0, epi=_epi, policy=dict(tile=_tile, splits=1))
    case(f"linear-{_fam}-t{_tile}-2src", linear_spec, M0, N0, 192, 16, epi="res", policy=dict(tile=_tile, splits=1))
    if _tile < 8:
        case(f"linear-ring-t{_tile}-splitk{RING_SPLITS[_tile]}", linear_spec, M0, N0, K0, epi="res",
             policy=dict(tile=_tile, splits=RING_SPLITS[_tile]))
        case(f"linear-ring-t{_tile}-geglu", linear_spec, M0, 384, K0, epi="geglu", policy=dict(tile=_tile, splits=1))
for _epi in ("bias", "res", "rowbias", "gelu"):
    case(f"linear-p8-t10-{_epi}", linear_spec, 200, 640, K0, epi=_epi, policy=dict(tile=10, splits=1),
         kernel=((200, 640, K0, 0), "gemm_p8<128x320"))
case("linear-p8-t10-2src", linear_spec, 200, 640, 192, 16, epi="res", policy=dict(tile=10, splits=1))
case("linear-p8-t8-geglu", linear_spec, M0, 640, K0, epi="geglu", policy=dict(tile=8, splits=1),
     kernel=((M0, 640, K0, 1), "gemm_p8<256x256,geglu"))
case("linear-p8-persist-w320-res", linear_spec, 4680, 4480, 128, epi="res", policy=dict(bn=320, persist=True),
     kernel=((4680, 4480, 128, 0), "128x320,persist>"))
case("linear-p8-persist-w256-geglu", linear_spec, 5448, 6144, 128, epi="geglu", policy=dict(bn=256, persist=True),
     kernel=((5448, 6144, 128, 1), "geglu,persist>"))
for _epi in ("bias", "res", "rowbias"):
    case(f"linear-rows-{_epi}", linear_spec, 3, 104, 40, epi=_epi, div=8, kernel=((3, 104, 40, 0), "gemm_rows"))
case("linear-skinny", linear_spec, 1030, 48, 640, epi="none", policy=dict(tile=5),
     kernel=((1030, 48, 640, 0), "gemm_skinny"))
for _bn in (192, 256, 320):
    case(f"linear_lora-w{_bn}", lora_spec, M0, K0, 640, 32, 640, 16, _bn)
for _lora in (False, True):
    case(f"linear_cross_attention-lora{int(_lora)}", xattn_spec, 3, 256, 128, 136, 77, 2, _lora)
case("linear_temporal_attention-h2d40", tattn_fused_spec, 2, 16, 16, 128, 2, 40)
case("linear_temporal_attention-h1d80", tattn_fused_spec, 2, 16, 16, 128, 1, 80)

CONV_RING = [(2, 1), (1, 4), (2, 3), (3, 1), (4, 1), (6, 1), (6, 2), (7, 1), (7, 3)]  # test_conv_tile_and_splitk_variants
for _mode, _mkw in (("s1", {}), ("s2", dict(stride=2)), ("up", dict(up=True))):
    for _ch, (_c1, _c2, _co) in (("64to320", (64, 0, 320)), ("64+64to128", (64, 64, 128))):
        for _tile, _sp in CONV_RING + [(0, 0)]:
            case(f"conv3x3-{_ch}-{_mode}-t{_tile}s{_sp}", conv_spec, 2, 9, 9, _c1, _c2, _co,
                 policy=dict(tile=_tile, splits=_sp, p8conv=True), **_mkw)
case("conv3x3-p8-s1", conv_spec, 2, 91, 91, 64, 0, 320, policy=dict(p8conv=True),
     kernel=((16562, 320, 576, 2), "gemm_p8<128x320,conv>"))
case("conv3x3-p8-s2", conv_spec, 2, 181, 181, 64, 0, 320, stride=2, policy=dict(p8conv=True),
     kernel=((16562, 320, 576, 2), "gemm_p8<128x320,conv>"))
case("conv3x3-p8-up", conv_spec, 2, 46, 45, 64, 0, 320, up=True, policy=dict(p8conv=True),
     kernel=((16560, 320, 576, 2), "gemm_p8<128x320,conv>"))
case("conv3x3-p8-2src", conv_spec, 2, 91, 91, 64, 64, 320, policy=dict(p8conv=True),
     kernel=((16562, 320, 1152, 2), "gemm_p8<128x320,conv>"))
case("conv3x3_down_pad0", conv_down_pad0_spec, 2, 9, 9, 64, 128)

for _on in (True, False):
    case(f"spatial_attention-self-sa{int(_on)}", spatial_spec, 2, 2, 200, 200, 1, _on)
    case(f"spatial_attention-cross-sa{int(_on)}", spatial_spec, 2, 2, 100, 77, 2, _on)
case("temporal_attention-3x5x7x64", temporal_spec, 3, 5, 7, 64)
case("temporal_attention-1x16x8x80", temporal_spec, 1, 16, 8, 80)

for _rows in (70, 300):
    for _C in (64, 320):
        for _silu in (False, True):
            case(f"group_norm-{_rows}x{_C}-silu{int(_silu)}", group_norm_spec, _rows, _C, _silu)
        case(f"group_norm_apply_partials-{_rows}x{_C}", gn_partials_spec, _rows, _C)
        case(f"layer_norm-{_rows}x{_C}", layer_norm_spec, _rows, _C, False)
        case(f"layer_norm_lora-{_rows}x{_C}", layer_norm_spec, _rows, _C, True)
        for _op in ("add_row_table", "permute_rows", "transpose", "copy2d", "softmax_rows", "gemm_f32out"):
            case(f"{_op}-{_rows}x{_C}", rowop_spec, _op, _rows, _C)
        case(f"layer_norm_bwd-{_rows}x{_C}", layer_norm_bwd_spec, _rows, _C)
        case(f"group_norm_bwd-{_rows}x{_C}", group_norm_bwd_spec, _rows, _C, _C == 320)
        case(f"geglu_bwd-{_rows}x{_C}", geglu_bwd_spec, _rows, _C)
case("linear_tn-direct", linear_tn_spec, 300, 136, 200)
case("linear_tn-split", linear_tn_spec, 4100, 136, 136)
case("colsum", colsum_spec, 1000, 64)
case("spatial_attention_bwd-self", spatial_bwd_spec, 2, 2, 200, 200, 1)
case("spatial_attention_bwd-cross", spatial_bwd_spec, 2, 2, 100, 77, 2)
case("temporal_attention_bwd-3x5x7x64", temporal_bwd_spec, 3, 5, 7, 64)
case("temporal_attention_bwd-1x16x8x80", temporal_bwd_spec, 1, 16, 8, 80)
for _op in ("zero_insert", "sumpool2x2"):
    case(f"{_op}-3x5x7x64", sampler_dgrad_spec, _op, 3, 5, 7, 64)
    case(f"{_op}-2x8x8x320", sampler_dgrad_spec, _op, 2, 8, 8, 320)


@pytest.mark.parametrize("cid", list(CASES))
def test_view_contract(cuda, K, cid):
    fn, a, kw = CASES[cid]
    run_case(K, cuda, fn(*a, **kw))


# ---------------------------------------------------------------- out= validation
# one case per wrapper that takes an output: (case id, the output arguments to damage)
OUT_ARGS = [
    ("linear-ring-t1-bias", "out"), ("linear_lora-w192", "out"), ("linear_cross_attention-lora0", "out"),
    ("linear_temporal_attention-h2d40", "out"), ("conv3x3-64to320-s1-t0s0", "out"), ("conv3x3_down_pad0", "out"),
    ("spatial_attention-cross-sa1", "out"), ("spatial_attention-cross-sa1", "lse"),
    ("temporal_attention-3x5x7x64", "out"), ("group_norm-70x64-silu0", "out"),
    ("group_norm_apply_partials-70x64", "out"), ("layer_norm-70x64", "out"), ("layer_norm_lora-70x64", "out"),
    ("layer_norm_lora-70x64", "u"), ("add_row_table-70x64", "out"), ("permute_rows-70x64", "out"),
    ("transpose-70x64", "out"), ("copy2d-70x64", "out"), ("softmax_rows-70x64", "out"), ("gemm_f32out-70x64", "out"),
    ("linear_tn-direct", "out"), ("geglu_bwd-70x64", "out"), ("colsum", "out"),
    ("spatial_attention_bwd-cross", "dq"), ("spatial_attention_bwd-cross", "dkv"),
    ("temporal_attention_bwd-3x5x7x64", "out"),
]


@pytest.mark.parametrize("damage", ["narrow", "dtype"])
@pytest.mark.parametrize("cid,arg", OUT_ARGS)
def test_out_argument_is_validated(cuda, K, cid, arg, damage):
    """A wrapper handed an output of the wrong width (a narrower view of a full-size arena: nothing outside owned
    memory could be touched even without the check) or of the wrong dtype raises VstError before any launch, and
    every output arena keeps its sentinel."""
    fn, a, kw = CASES[cid]
    spec = fn(*a, **kw)
    t, arenas = materialize(spec, cuda, True)
    rows, cols, dtype, kind = spec.outs[arg]
    if damage == "narrow":
        t[arg] = t[arg][:-8] if kind == "vec" else t[arg][:, :cols - 8]
    else:
        other = F32 if dtype == BF16 else BF16
        v, full = arena(rows, cols, other, "sentinel", cuda)
        t[arg] = v[0] if kind == "vec" else v
        arenas[arg + ":other dtype"] = (full, GUARD_TOP, GUARD_COL, rows, cols)
    with policy(K, **spec.policy):
        with pytest.raises(K._lib.VstError, match=arg):
            spec.run(K, t)
    torch.cuda.synchronize()
    for name, (full, r0, c0, nr, nc) in arenas.items():
        verify_out(name, full, r0, c0, nr, nc, untouched=True)


def test_elementwise_out_is_validated(cuda, K):
    """silu / add address every operand as one flat block: an out of another size, dtype or layout is refused."""
    a, b = torch.zeros(16, 64, dtype=BF16, device=cuda), torch.zeros(16, 64, dtype=BF16, device=cuda)
    v, full = arena(16, 64, BF16, "sentinel", cuda)
    f32, full32 = dense(16, 64, F32, "sentinel", cuda)
    for bad in (v, full[:8, :64], f32, full[:32].reshape(-1)[:16 * 64 - 8]):
        with pytest.raises(K._lib.VstError, match="out"):
            K.add(a, b, out=bad)
        with pytest.raises(K._lib.VstError, match="out"):
            K.silu(a, out=bad)
    torch.cuda.synchronize()
    verify_out("bf16 arena", full, GUARD_TOP, GUARD_COL, 16, 64, untouched=True)
    verify_out("fp32 buffer", full32, GUARD_TOP, 0, 16, 64, untouched=True)
