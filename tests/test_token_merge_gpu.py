"""Token merging on the GPU: the matching against tests/test_token_merge.py's fp64 `tome_ref`, the
merge and the unmerge against fp64 on the kernel's own plans (strided views inside poisoned guard bands), batch
independence and determinism, one spatial BasicTransformerBlock against an fp32 CPU restatement of the ToMe block that
uses the plan the kernel recorded, and the option through the UNet and the denoiser.

Bars.  Scores: |best - best_ref| <= (C + 16) 2^-24, the worst-case fp32 dot-product bound for unit vectors in any
summation order.  With tau = 2 (C + 16) 2^-24 a source is decided when its top-two score gap is >= tau and its best is
>= tau clear of the selection cut; decided sources match the reference exactly, undecided ones pick a destination whose
reference score is within tau of the reference maximum, and at most 5 % of an image's sources are undecided.  Merge /
unmerge: |got - ref| <= 2^-8 |ref| + 2^-8 max|x| over the row's members (one bf16 rounding of an fp32 sum).  Block:
e <= 3e-2 and e <= 1.25 e0 + 2e-3 with e0 the same block's error with merging off, the form
tests/test_cross_frame_gpu.py uses.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 0x7FA5  # a bf16 NaN pattern no kernel produces


@pytest.fixture(scope="module")
def K():
    from video_style_transfer_amd import kernels
    return kernels


def sizes(H, W, ratio):
    from video_style_transfer_amd import kernels
    return kernels.tome_sizes(H, W, 2, 2, ratio)


@functools.lru_cache(maxsize=None)
def inputs(nimg, H, W, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + nimg * H * W + C)
    return torch.randn(nimg * H * W, C, generator=g).to(BF16)


@functools.lru_cache(maxsize=None)
def reference(nimg, H, W, C, r, seed=0, offsets=None):
    """tome_ref of every image of inputs(...), computed once and shared (never modified)."""
    from test_token_merge import tome_ref
    x = inputs(nimg, H, W, C, seed).view(nimg, H * W, C)
    off = None if offsets is None else torch.tensor(offsets).view(H // 2, W // 2)
    return [tome_ref(x[i], H, W, r, offsets=off) for i in range(nimg)]


def parse(plan, N, Nd, Ns, r):
    """One image's plan row (CPU int32 [6 N + 4]) by the layout of include/vst.h."""
    import types
    start = plan[3 * N:3 * N + Nd + 1]
    return types.SimpleNamespace(slot=plan[:N].long(), dst_tok=plan[N:N + Nd].long(), src_tok=plan[N + Nd:2 * N].long(),
                                 node=plan[2 * N:2 * N + Ns].long(), start=start.long(),
                                 list=plan[3 * N + Nd + 1:3 * N + Nd + 1 + r].long(),
                                 kept_tok=plan[4 * N + 4:4 * N + 4 + Ns - r].long())


def run_match(K, cuda, x, nimg, H, W, r, seed=None, step=0, layer=0):
    N = H * W
    plan = K.tome_plan(nimg, N, cuda)
    kw = {}
    if seed is not None:
        kw = dict(seed=torch.tensor([seed], dtype=torch.int64, device=cuda),
                  step_idx=torch.tensor([step], dtype=torch.int32, device=cuda), layer=layer)
    best = K.tome_match(x.to(cuda), nimg, H, W, r, plan, **kw)
    torch.cuda.synchronize()
    return plan, best


def check_plan(p, ref_dst, N, Nd, Ns, r):
    """A valid partition with exactly r merged sources and the stated row layout."""
    assert p.dst_tok.tolist() == ref_dst.tolist()
    is_dst = torch.zeros(N, dtype=torch.bool)
    is_dst[p.dst_tok] = True
    assert p.src_tok.tolist() == torch.nonzero(~is_dst).reshape(-1).tolist()
    assert p.slot[p.dst_tok].tolist() == list(range(Nd))
    assert int(p.node.min()) >= 0 and int(p.node.max()) < Nd
    s_slot = p.slot[p.src_tok]
    merged = s_slot < Nd
    assert int(merged.sum()) == r
    assert torch.equal(s_slot[merged], p.node[merged])
    kept = p.src_tok[~merged]
    assert s_slot[~merged].tolist() == list(range(Nd, N - r))          # ascending token index
    assert p.kept_tok.tolist() == kept.tolist()
    assert int(p.slot.min()) == 0 and int(p.slot.max()) == N - r - 1
    # member lists: CSR over the destinations, tokens ascending inside each
    assert int(p.start[0]) == 0 and int(p.start[Nd]) == r and bool((p.start[1:] >= p.start[:-1]).all())
    mt, mn = p.src_tok[merged], p.node[merged]
    order = torch.argsort(mn * N + mt)
    assert p.list.tolist() == mt[order].tolist()
    assert torch.equal(torch.bincount(mn, minlength=Nd), p.start[1:] - p.start[:-1])
    return merged


# ------------------------------------------------------------------ 1. the matching against tome_ref
CASES = [(2, 4, 4, 64, .5), (2, 5, 7, 128, .25), (4, 16, 16, 1280, .5), (2, 32, 32, 640, .5), (1, 64, 64, 640, .5),
         (2, 32, 32, 640, .75), (2, 16, 16, 64, 1.0 / 256)]


@pytest.mark.parametrize("nimg,H,W,C,ratio", CASES)
def test_match_vs_reference(cuda, K, nimg, H, W, C, ratio):
    N, Nd, Ns, r = sizes(H, W, ratio)
    if ratio == .75:
        assert r == Ns                     # the clamp
    if ratio < .01:
        assert r == 1
    x = inputs(nimg, H, W, C)
    plan, best = run_match(K, cuda, x, nimg, H, W, r)
    plan, best = plan.cpu(), best.cpu().to(F64)
    bound = (C + 16) * 2.0 ** -24
    tau = 2 * bound
    refs = reference(nimg, H, W, C, r)
    for i, ref in enumerate(refs):
        p = parse(plan[i], N, Nd, Ns, r)
        merged = check_plan(p, ref.dst_tok, N, Nd, Ns, r)
        err = (best[i] - ref.best).abs().max().item()
        top2 = ref.scores.topk(2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
        clear = torch.ones(Ns, dtype=torch.bool)
        if 0 < r < Ns:
            sb = ref.best.sort(descending=True).values
            last_in, first_out = sb[r - 1], sb[r]
            clear = torch.where(ref.merged, ref.best - first_out >= tau, last_in - ref.best >= tau)
        decided = (gap >= tau) & clear
        und = 1.0 - decided.double().mean().item()
        print(f"[tome] match {nimg}x{H}x{W}x{C} r={r} img {i}: |best - ref| max {err:.3e} (bound {bound:.3e}), "
              f"undecided {100 * und:.2f} %")
        assert err <= bound, (err, bound)
        assert torch.equal(merged[decided], ref.merged[decided])
        assert torch.equal(p.node[decided], ref.node[decided])
        picked = ref.scores.gather(1, p.node[:, None])[:, 0]
        assert bool((picked >= ref.best - tau).all())
        assert und <= 0.05, und


def test_match_use_rand(cuda, K):
    """The destination draw: one pattern for every image, another at another step, every destination inside its cell,
    and the host restatement (token_merge.destination_offsets) bit for bit; the matching holds on that pattern."""
    from video_style_transfer_amd.token_merge import destination_offsets, destination_tokens
    nimg, H, W, C = 3, 8, 10, 64
    N, Nd, Ns, r = sizes(H, W, .5)
    x = inputs(nimg, H, W, C)
    seen = {}
    for step in (0, 1):
        plan, best = run_match(K, cuda, x, nimg, H, W, r, seed=2 ** 40 + 11, step=step, layer=7)
        plan = plan.cpu()
        ps = [parse(plan[i], N, Nd, Ns, r) for i in range(nimg)]
        for p in ps[1:]:
            assert torch.equal(p.dst_tok, ps[0].dst_tok)
        d = ps[0].dst_tok
        cells = torch.arange(Nd)
        assert torch.equal((d // W) // 2, cells // (W // 2)) and torch.equal((d % W) // 2, cells % (W // 2))
        off = destination_offsets(H, W, 2, 2, 2 ** 40 + 11, step, 7)
        assert torch.equal(d, destination_tokens(H, W, 2, 2, off))
        seen[step] = d
        refs = reference(nimg, H, W, C, r, 0, tuple(off.reshape(-1).tolist()))
        for i, ref in enumerate(refs):
            merged = check_plan(ps[i], ref.dst_tok, N, Nd, Ns, r)
            assert (best[i].cpu().to(F64) - ref.best).abs().max().item() <= (C + 16) * 2.0 ** -24
    assert not torch.equal(seen[0], seen[1])
    assert len(set((seen[0] % W % 2 + 2 * (seen[0] // W % 2)).tolist())) > 1   # not all top-left


def test_zero_rows_score_zero(cuda, K):
    nimg, H, W, C = 1, 4, 4, 64
    x = inputs(nimg, H, W, C).clone()
    x[1] = 0          # a source
    x[2] = 0          # a destination
    plan, best = run_match(K, cuda, x, nimg, H, W, 6)
    assert torch.isfinite(best).all()
    assert best[0, 0].item() == 0.0   # source token 1 is source 0


# ------------------------------------------------------------------ 2. merge and unmerge_add on the kernel's plans
def nan_arena(t, dev, top=8, bottom=24, side=8):
    rows, cols = t.shape
    ld = (side + cols + side + 7) // 8 * 8
    a = torch.full((top + rows + bottom, ld), float("nan"), dtype=t.dtype, device=dev)
    v = a[top:top + rows, side:side + cols]
    v.copy_(t)
    return v


def out_arena(rows, cols, dev, top=8, bottom=24, side=8):
    ld = (side + cols + side + 7) // 8 * 8
    a = torch.empty((top + rows + bottom, ld), dtype=BF16, device=dev)
    a.view(torch.int16).fill_(SENT)
    return a[top:top + rows, side:side + cols], a, (top, side)


def verify_arena(name, full, origin, rows, cols):
    same = full.view(torch.int16) == SENT
    outside = ~same
    outside[origin[0]:origin[0] + rows, origin[1]:origin[1] + cols] = False
    assert not outside.any(), f"{name}: written outside the view at {outside.nonzero()[:4].tolist()}"
    assert not same[origin[0]:origin[0] + rows, origin[1]:origin[1] + cols].any(), f"{name}: unwritten elements"
    assert torch.isfinite(full[origin[0]:origin[0] + rows, origin[1]:origin[1] + cols].float()).all(), name


@pytest.mark.parametrize("nimg,H,W,C,ratio", [(2, 4, 4, 64, .5), (2, 5, 7, 128, .25), (2, 32, 32, 640, .5),
                                              (2, 16, 16, 1280, .75)])
def test_merge_and_unmerge_vs_fp64(cuda, K, nimg, H, W, C, ratio):
    N, Nd, Ns, r = sizes(H, W, ratio)
    Nm = N - r
    x = inputs(nimg, H, W, C)
    xv = nan_arena(x, cuda)
    plan = K.tome_plan(nimg, N, cuda)
    best = K.tome_match(xv, nimg, H, W, r, plan)
    plan0, best0 = run_match(K, cuda, x, nimg, H, W, r)
    assert torch.equal(plan, plan0) and torch.equal(best, best0)       # guard columns are not read
    slot = plan[:, :N].cpu().long()
    y, full, org = out_arena(nimg * Nm, C, cuda)
    K.tome_merge(xv, nimg, H, W, r, plan, out=y)
    torch.cuda.synchronize()
    verify_arena("merge", full, org, nimg * Nm, C)
    assert torch.equal(y, K.tome_merge(x.to(cuda), nimg, H, W, r, plan))
    y = y.cpu()
    x64 = x.to(F64).view(nimg, N, C)
    for i in range(nimg):
        cnt = torch.bincount(slot[i], minlength=Nm)
        assert int(cnt.min()) >= 1
        ref = torch.zeros(Nm, C, dtype=F64).index_add_(0, slot[i], x64[i]) / cnt[:, None]
        amax = torch.zeros(Nm, dtype=F64).scatter_reduce_(0, slot[i], x64[i].abs().amax(dim=1), "amax")
        got = y[i * Nm:(i + 1) * Nm]
        tol = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * amax[:, None]
        err = (got.to(F64) - ref).abs()
        print(f"[tome] merge {nimg}x{H}x{W}x{C} r={r} img {i}: max err/tol {(err / tol.clamp_min(1e-300)).max():.3f}")
        assert bool((err <= tol).all())
        single = cnt == 1
        owner = torch.zeros(Nm, dtype=torch.long).scatter_(0, slot[i], torch.arange(N))
        assert torch.equal(got[single].view(torch.int16), x.view(nimg, N, C)[i][owner[single]].view(torch.int16))
    # unmerge_add: with a residual, in place on the residual, and plain
    g = torch.Generator().manual_seed(5)
    o = torch.randn(nimg * Nm, C, generator=g).to(BF16)
    res = torch.randn(nimg * N, C, generator=g).to(BF16)
    ov, rv = nan_arena(o, cuda), nan_arena(res, cuda)
    z, full, org = out_arena(nimg * N, C, cuda)
    K.tome_unmerge_add(ov, nimg, N, r, plan, residual=rv, out=z)
    torch.cuda.synchronize()
    verify_arena("unmerge_add", full, org, nimg * N, C)
    idx = (slot + torch.arange(nimg)[:, None] * Nm).reshape(-1)
    ref = res.to(F64) + o.to(F64)[idx]
    amax = torch.maximum(res.to(F64).abs().amax(dim=1), o.to(F64)[idx].abs().amax(dim=1))
    assert bool(((z.cpu().to(F64) - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -8 * amax[:, None]).all())
    K.tome_unmerge_add(ov, nimg, N, r, plan, residual=rv, out=rv)       # y aliases res
    assert torch.equal(rv, z)
    p, full, org = out_arena(nimg * N, C, cuda)
    K.tome_unmerge_add(ov, nimg, N, r, plan, out=p)
    torch.cuda.synchronize()
    verify_arena("unmerge", full, org, nimg * N, C)
    assert torch.equal(p.cpu().view(torch.int16), o[idx].view(torch.int16))


# ------------------------------------------------------------------ 3. batch independence and determinism
@pytest.mark.parametrize("H,W,C,seed", [(16, 16, 1280, None), (9, 11, 128, 77)])
def test_batch_independent_and_deterministic(cuda, K, H, W, C, seed):
    nimg = 4
    N, Nd, Ns, r = sizes(H, W, .5)
    x = inputs(nimg, H, W, C).to(cuda)
    g = torch.Generator().manual_seed(9)
    o = torch.randn(nimg * (N - r), C, generator=g).to(BF16).to(cuda)

    def run(x, o, n):
        plan, best = run_match(K, cuda, x, n, H, W, r, seed=seed, step=3, layer=2)
        m = K.tome_merge(x, n, H, W, r, plan)
        u = K.tome_unmerge_add(o, n, N, r, plan, residual=x)
        return plan, best, m, u
    a, b = run(x, o, nimg), run(x, o, nimg)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    sub = run(x[2 * N:].contiguous(), o[2 * (N - r):].contiguous(), 2)
    assert torch.equal(sub[0], a[0][2:]) and torch.equal(sub[1], a[1][2:])
    assert torch.equal(sub[2], a[2][2 * (N - r):]) and torch.equal(sub[3], a[3][2 * N:])


def test_refused_before_any_launch(cuda, K):
    VstError = K._lib.VstError
    x = inputs(1, 4, 4, 64).to(cuda)
    plan = K.tome_plan(1, 16, cuda)
    K.profile_launches(True)
    try:
        with pytest.raises(VstError):
            K.tome_match(x, 1, 4, 4, 13, plan)                        # r > Ns
        with pytest.raises(VstError):
            K.tome_match(x[:, :40], 1, 4, 4, 2, plan)                 # C % 64
        with pytest.raises(VstError):
            K.tome_match(x, 1, 4, 4, 2, plan, seed=torch.zeros(1, dtype=torch.int64, device=cuda))
        with pytest.raises(VstError):
            K.tome_match(x, 1, 4, 4, 2, K.tome_plan(1, 20, cuda))     # a plan of another size
        with pytest.raises(VstError):
            K.tome_match(x.cpu(), 1, 4, 4, 2, plan)
        with pytest.raises(VstError):
            K.tome_merge(x, 1, 4, 4, 2, plan, out=torch.empty(16, 64, dtype=BF16, device=cuda))
        with pytest.raises(VstError):
            K.tome_unmerge_add(x, 1, 16, 16, plan)
        with pytest.raises(VstError):
            K.tome_match(torch.empty(128 * 64, 64, dtype=BF16, device=cuda), 1, 128, 64, 2, K.tome_plan(1, 8192, cuda))
        assert K.collect_launches() == []
    finally:
        K.profile_launches(False)


# ------------------------------------------------------------------ 4. one spatial block against fp32
HEADS, CROSS, L = 10, 256, 77


@pytest.fixture(scope="module")
def block(cuda):
    """A spatial BasicTransformerBlock, C = 640, 10 heads of 64, UnZipLoRA rank 8; weights bf16 on the device (the LoRA
    factors fp32, as the models keep them) and their fp32 copies under the oracle's names."""
    from video_style_transfer_amd.unet_motion import BasicTransformerBlock
    from video_style_transfer_amd.utils import attach_unziplora_layers
    torch.manual_seed(22)
    holder = torch.nn.Module()
    holder.blk = BasicTransformerBlock(640, HEADS, 64, CROSS)
    attach_unziplora_layers(holder, 8)
    with torch.no_grad():
        for name, p in holder.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
            if "lora_layer" not in name:
                p.copy_(p.to(BF16).float())
    holder.requires_grad_(False)
    P = {k: v.clone().float() for k, v in holder.state_dict().items()}
    for name, p in holder.named_parameters():
        if "lora_layer" not in name:
            p.data = p.data.to(BF16)
    holder.to(cuda)
    return holder.blk, P


def scaled(P, gc, gs):
    out = dict(P)
    for k, v in P.items():
        if k.endswith("content_up.weight"):
            out[k] = v * gc
        elif k.endswith("style_up.weight"):
            out[k] = v * gs
    return out


def tome_block_ref(P, x, enc, slot, r, merge_attn, merge_mlp, cross=None):
    """fp32 restatement of the ToMe block on x [nimg, N, C] with the recorded slot [nimg, N] (None: the plain block).
    cross = (frames per clip, sources): attn1 is the cross-frame attention of tests/test_cross_frame.py's frames_ref."""
    import oracle.unet as OU
    from oracle.unet import LoRAState
    lora = LoRAState()
    nimg, N, C = x.shape

    def merge(t):
        Nm = N - r
        out = torch.zeros(nimg, Nm, C)
        cnt = torch.zeros(nimg, Nm)
        for i in range(nimg):
            out[i].index_add_(0, slot[i], t[i])
            cnt[i] = torch.bincount(slot[i], minlength=Nm)
        return out / cnt[..., None]

    def unmerge(o):
        return torch.stack([o[i][slot[i]] for i in range(nimg)])

    def attn1(t):
        if cross is None:
            return OU.attention(P, "blk.attn1", t, None, HEADS, lora)
        from test_cross_frame import frames_ref
        Fr, sources = cross
        n = t.shape[1]
        q, k, v = (OU.proj(P, f"blk.attn1.{w}", t, lora).reshape(nimg * n, -1) for w in ("to_q", "to_k", "to_v"))
        return OU.proj(P, "blk.attn1.to_out.0", frames_ref(q, k, v, nimg // Fr, Fr, n, HEADS, sources).view(nimg, n, -1),
                       lora)

    n = OU.layer_norm(P, "blk.norm1", x)
    if slot is not None and merge_attn:
        x = x + unmerge(attn1(merge(n)))
    else:
        x = x + attn1(n)
    n = OU.layer_norm(P, "blk.norm2", x)
    x = x + OU.attention(P, "blk.attn2", n, enc, HEADS, lora)
    n = OU.layer_norm(P, "blk.norm3", x)
    if slot is not None and merge_mlp:
        return x + unmerge(OU.geglu_ff(P, "blk.ff", merge(n)))
    return x + OU.geglu_ff(P, "blk.ff", n)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def run_block(K, cuda, blk, x, enc, H, W, Fr, tm, gate=None, cross_frame=None):
    from video_style_transfer_amd.unet_motion import ForwardOptions, FwdCtx
    nimg, N, C = x.shape
    ctx = FwdCtx(nimg // Fr, Fr, None, enc.to(cuda), {},
                 opts=ForwardOptions(cross_frame=cross_frame, lora_gate=gate, token_merging=tm),
                 latent_hw=(2 * H, 2 * W), spatial_hw=(H, W))
    with K.row_invariant():
        out = blk.run(x.reshape(nimg * N, C).to(cuda), nimg, N, ctx)
    torch.cuda.synchronize()
    return out.view(nimg, N, C)


@pytest.mark.parametrize("H,mlp,variant", [(16, False, "plain"), (16, True, "plain"), (32, False, "plain"),
                                           (32, True, "plain"), (16, True, "gates"), (16, True, "cross_frame")])
def test_block_vs_fp32(cuda, K, block, H, mlp, variant):
    from video_style_transfer_amd.lora_gate import LoraGate
    from video_style_transfer_amd.token_merge import TokenMerging
    from video_style_transfer_amd.unet_motion import CrossFrameAttention
    blk, P = block
    W, C, Fr, nimg = H, 640, 2, 2
    N = H * W
    g = torch.Generator().manual_seed(H + mlp)
    x = torch.randn(nimg, N, C, generator=g).to(BF16)
    enc = torch.randn(1, L, CROSS, generator=g).to(BF16)
    tm = TokenMerging(ratio=0.5, use_rand=True, merge_mlp=mlp)
    tm.bind(torch.tensor([1234], dtype=torch.int64, device=cuda), torch.tensor([3], dtype=torch.int32, device=cuda))
    gate, pairs, cf, cross = None, [(1.0, 1.0)] * nimg, None, None
    if variant == "gates":
        pairs = [(0.5, 1.5), (1.25, 0.0)]
        gate = LoraGate(nimg, cuda).set([p[0] for p in pairs], [p[1] for p in pairs])
    if variant == "cross_frame":
        cf, cross = CrossFrameAttention(("first",)), (Fr, ("first",))

    def ref(slot, r):
        if cross is not None:
            return tome_block_ref(P, x.float(), enc.float(), slot, r, True, mlp, cross)
        # (images are independent: each with its own gate pair folded into the up factors)
        return torch.cat([tome_block_ref(scaled(P, *pairs[i]), x[i:i + 1].float(), enc.float(),
                                         None if slot is None else slot[i:i + 1], r, True, mlp)
                          for i in range(nimg)])
    out0 = run_block(K, cuda, blk, x, enc, H, W, Fr, None, gate, cf)
    e0 = rel(out0, ref(None, 0))
    K.profile_launches(True)
    try:
        out = run_block(K, cuda, blk, x, enc, H, W, Fr, tm, gate, cf)
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert kinds.count("tome_match") == 1 and kinds.count("tome_merge") == kinds.count("tome_unmerge_add") == 1 + mlp
    st = tm.layers[0]                                                    # the test hook: the recorded plan
    assert (st.N, st.r, st.nimg) == (N, N // 2, nimg)
    e = rel(out, ref(st.slot().cpu().long(), st.r))
    print(f"[tome] block N={N} mlp={mlp} {variant}: rel_l2={e:.3e}, merging off {e0:.3e}")
    assert e <= 3e-2 and e <= 1.25 * e0 + 2e-3, (e, e0)
    assert rel(out, out0) > 1e-2                                         # the option does something
    # off and ratio 0: the plain block's launches, bit for bit
    assert torch.equal(run_block(K, cuda, blk, x, enc, H, W, Fr, TokenMerging(ratio=0.0), gate, cf), out0)
    assert torch.equal(run_block(K, cuda, blk, x, enc, H, W, Fr, TokenMerging(max_downsample=1), gate, cf), out0)


def test_block_refuses_another_processor_and_autograd(cuda, K, block):
    from video_style_transfer_amd.attention_processor import AttnProcessor2_0
    from video_style_transfer_amd.token_merge import TokenMerging
    blk, _ = block
    x = torch.zeros(2, 64, 640, dtype=BF16)
    enc = torch.zeros(1, L, CROSS, dtype=BF16)
    keep = blk.attn1.processor
    blk.attn1.set_processor(AttnProcessor2_0())
    K.profile_launches(True)
    try:
        with pytest.raises(K._lib.VstError, match="AnimateDiffAttnProcessor2_0"):
            run_block(K, cuda, blk, x, enc, 8, 8, 2, TokenMerging())
        blk.attn1.set_processor(keep)
        from video_style_transfer_amd.unet_motion import ForwardOptions, FwdCtx
        xg = x.reshape(128, 640).to(cuda).requires_grad_(True)
        with pytest.raises(K._lib.VstError, match="inference only"):
            blk.run(xg, 2, 64, FwdCtx(1, 2, None, enc.to(cuda), {}, opts=ForwardOptions(token_merging=TokenMerging()),
                                      latent_hw=(16, 16), spatial_hw=(8, 8)))
        assert K.collect_launches() == []
    finally:
        blk.attn1.set_processor(keep)
        K.profile_launches(False)


# ------------------------------------------------------------------ 5. the UNet and the denoiser
@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16)
    unet = build_unet(cfg, state_dict=sd, device=cuda)
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)})
    return dict(cfg=cfg, lat=lat, enc=enc, pooled=pooled, unet=unet, kw=kw)


def test_unet_off_and_ratio_zero_are_todays_forward(cuda, K, tiny):
    from video_style_transfer_amd.token_merge import TokenMerging
    unet, lat, enc, kw = tiny["unet"], tiny["lat"].to(cuda), tiny["enc"].to(cuda), tiny["kw"]
    t = torch.tensor([761.0, 761.0], device=cuda)
    base = unet(lat, t, enc, **kw).sample
    assert torch.equal(unet(lat, t, enc, token_merging=None, **kw).sample, base)
    assert torch.equal(unet(lat, t, enc, token_merging=TokenMerging(ratio=0.0), **kw).sample, base)
    assert torch.equal(unet(lat, t, enc, token_merging=TokenMerging(max_downsample=1), **kw).sample, base)
    K.profile_launches(True)
    try:
        on = unet(lat, t, enc, token_merging=TokenMerging(max_downsample=4, merge_mlp=True), **kw).sample
        kinds = [r[0] for r in K.collect_launches()]
    finally:
        K.profile_launches(False)
    assert kinds.count("tome_match") == 17 and kinds.count("tome_merge") == 34   # every spatial block of the tiny model
    assert torch.isfinite(on).all() and not torch.equal(on, base)
    unet.enable_token_merging(ratio=0.5, max_downsample=4, merge_mlp=True)
    try:
        assert torch.equal(unet(lat, t, enc, **kw).sample, on)
    finally:
        unet.disable_token_merging()
    assert torch.equal(unet(lat, t, enc, **kw).sample, base)
    with pytest.raises(K._lib.VstError, match="merge_crossattn"):
        unet(lat, t, enc, token_merging=dict(merge_crossattn=True), **kw)


def test_denoiser_replay_equals_eager(cuda, tiny):
    """3 steps at tiny size with use_rand: the captured step replays the eager run's bits, so the destination pattern
    follows the device step counter under replay; and the pattern does change from step to step."""
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    from video_style_transfer_amd.token_merge import TokenMerging
    unet, enc, pooled = tiny["unet"], tiny["enc"], tiny["pooled"]
    outs, dsts = {}, {}
    for use_graph in (True, False):
        tm = TokenMerging(ratio=0.5, max_downsample=2, use_rand=True, merge_mlp=True)
        den = AnimateDiffDenoiser(unet, 4, 128, 128, num_inference_steps=10, device=cuda, use_graph=use_graph,
                                  token_merging=tm)
        den.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
        den.init_latents(seed=3)
        steps = []
        for _ in range(3):
            den.run_steps(1)
            st = next(iter(tm.layers.values()))
            steps.append(st.plan[0, st.N:st.N + st.Nd].clone())
        outs[use_graph], dsts[use_graph] = den.lat.clone(), steps
        assert (den.graph is not None) == use_graph and len(tm.layers) == 5   # the blocks of the 8 x 8 level
    assert torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], outs[False])
    for a, b in zip(dsts[True], dsts[False]):
        assert torch.equal(a, b)
    assert not torch.equal(dsts[True][0], dsts[True][1])
    plain = AnimateDiffDenoiser(unet, 4, 128, 128, num_inference_steps=10, device=cuda, use_graph=False)
    plain.set_prompt_embeds(enc[1:2], pooled[1:2], enc[0:1], pooled[0:1])
    plain.init_latents(seed=3)
    assert not torch.equal(plain.run_steps(3), outs[False])
