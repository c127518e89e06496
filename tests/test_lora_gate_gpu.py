"""Per-frame content / style strength on the GPU: the row gate on the LoRA down-projection u.

Kernel level: the gated lora_post of the 8-phase GEMM (every LoRA tile, the persistent 128x320 grid, the
cross-attention epilogue) and vst_lora_gate, mostly as exact statements -- the gate multiplies the already rounded u,
so a one-hot up-projection exposes bf16(g * u) bit for bit, and binary gates reproduce an ungated call whose V has
the gated-off columns zeroed.  Shapes are the smallest that reach every index the gate adds: K >= 128 (the in-GEMM
floor), an M tail, and a gate_div that changes the gate row inside a 16-row MFMA block.

Above the kernels: the attention processor (per-frame gates against uniform ones, frame by frame), the UNet against
fp32 restatements built from oracle.unet without editing it, and the denoiser (graph replay, new values under a
captured step, composition with the other options)."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K(cuda):
    from video_style_transfer_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def check(out, ref, rel_l2, rel_max, name=""):
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), name
    err = out - ref
    l2 = (err.norm() / ref.norm().clamp_min(1e-12)).item()
    mx = (err.abs().max() / ref.abs().max().clamp_min(1e-12)).item()
    print(f"[gate] {name}: rel_l2={l2:.3e} rel_max={mx:.3e}")
    assert l2 <= rel_l2 and mx <= rel_max, f"{name}: rel_l2={l2:.3e} rel_max={mx:.3e}"
    return l2, mx


def _operands(M, Kd, nproj, n_per, r_per, P, gen):
    """x [M, Kd]; Acat [P, Kd] (rows past nproj * r_per zero); W_aug [nproj * n_per, Kd + P] with projection i's up
    factors in columns Kd + i * r_per (the build_ops layout).  CPU tensors."""
    x = rnd(M, Kd, gen=gen)
    A = torch.zeros(P, Kd)
    A[: nproj * r_per] = torch.randn(nproj * r_per, Kd, generator=gen) * Kd ** -0.5
    N = nproj * n_per
    W = torch.zeros(N, Kd + P)
    W[:, :Kd] = torch.randn(N, Kd, generator=gen) * Kd ** -0.5
    for i in range(nproj):
        W[i * n_per:(i + 1) * n_per, Kd + i * r_per:Kd + (i + 1) * r_per] = \
            torch.randn(n_per, r_per, generator=gen) * r_per ** -0.5
    return x, A.to(BF), W.to(BF)


def _expand(pairs, keys):
    """[ng, 2] (content, style) gates -> [ng, len(keys)] by column key (-1: 1)."""
    t = torch.ones(pairs.shape[0], len(keys))
    for c, k in enumerate(keys):
        if k >= 0:
            t[:, c] = pairs[:, k]
    return t


def _zero_cols(W, Kd, keys, key):
    """W with the up-projection columns of `key` zeroed."""
    W = W.clone()
    for c, k in enumerate(keys):
        if k == key:
            W[:, Kd + c] = 0
    return W


# ----------------------------------------------------------------------------- the in-GEMM gate
@pytest.mark.parametrize("N,bn", [(192, 192), (192, 256), (320, 320)])
def test_gated_gemm_is_the_definition_bit_for_bit(cuda, K, N, bn):
    """Base weight zero and a one-hot V (V[n][c] = 1 for n == c < 16): output column c < 16 is u column c, so the
    ungated call returns the kernel's own bf16(u) and the gated call must return bf16(g * float(u)) exactly, for
    gates 0, 1, above 1, negative and fractional, different in every column; 600 = 2 x 256 + 88 rows (an M tail) in
    gate rows of 100 (a gate row changes inside a 16-row block, and inside a tile), K = 136 (a K tail)."""
    M, Kd, P, div = 600, 136, 32, 100
    g = torch.Generator().manual_seed(N + bn)
    x = rnd(M, Kd, gen=g)
    A = torch.zeros(P, Kd)
    A[:16] = torch.randn(16, Kd, generator=g) * Kd ** -0.5
    W = torch.zeros(N, Kd + P)
    for c in range(16):
        W[c, Kd + c] = 1.0
    ng = (M + div - 1) // div
    gate = torch.randn(ng, P, generator=g) * 1.5
    pick = torch.randint(0, 4, (ng, P), generator=g)
    gate = torch.where(pick == 0, torch.zeros(()), torch.where(pick == 1, torch.ones(()), gate))
    assert (gate == 0).any() and (gate == 1).any() and (gate > 1).any() and (gate < 0).any()
    xd, Ad, Wd, gd = x.to(cuda), A.to(BF).to(cuda), W.to(BF).to(cuda), gate.to(cuda)
    with K.p8_tile_width(bn):
        assert K.gemm_lora_tile(M, N, Kd, P, N, 16) == bn
        plain = K.linear_lora(xd, Wd, Ad, N, 16).cpu()
        K.profile_launches(True)
        gated = K.linear_lora(xd, Wd, Ad, N, 16, gate=gd, gate_div=div).cpu()
        rec = K.collect_launches()
        K.profile_launches(False)
    assert rec[0][1] == (f"gemm_p8<128x{bn},lora,gate>" if bn == 320 else f"gemm_p8<256x{bn},lora,gate>"), rec
    u = plain[:, :16]
    assert u.abs().max() > 0.5 and torch.equal(plain[:, 16:], torch.zeros(M, N - 16, dtype=BF))
    # (the kernel's u against torch's, so that `plain` really is the down-projection)
    check(u, x.float() @ A[:16].to(BF).float().t(), 5e-3, 1e-2, f"u {N}/{bn}")
    rows = torch.arange(M) // div
    want = (gate[rows, :16] * u.float()).to(BF)
    assert torch.equal(gated[:, :16], want)
    assert torch.equal(gated[:, 16:], torch.zeros(M, N - 16, dtype=BF))


QKV_KEYS = ((0,) * 8 + (1,) * 8) * 3 + (-1,) * 16       # stacked q/k/v, UnZipLoRA r = 8, both terms: P = 64
CONTENT_KEYS = (0,) * 24 + (-1,) * 8                    # the content-only layout: 8-column groups, P = 32


@pytest.mark.parametrize("keys,gr,P", [(QKV_KEYS, 16, 64), (CONTENT_KEYS, 8, 32)])
def test_binary_gates_select_rows_and_columns(cuda, K, keys, gr, P):
    """Per gate row one of (1,1), (1,0), (0,1), (0,0): every row group equals, bit for bit, the same rows of the
    ungated call whose V has the switched-off key's columns zeroed (a zero u column and a zero V column add the
    same exact zeros); with bias and residual; ub0 = 0, 16, 32 (QKV) and 8-column groups inside one block
    (content-only).  Gates of 1 everywhere are the ungated call."""
    M, Kd, n_per, div = 600, 136, 256, 100
    g = torch.Generator().manual_seed(gr)
    x, A, W = _operands(M, Kd, 3, n_per, gr, P, g)
    N = 3 * n_per
    b = (torch.randn(N, generator=g) * 0.1).to(cuda)
    r = rnd(M, N, gen=g).to(cuda)
    ng = (M + div - 1) // div
    pairs = torch.tensor([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 1.0], [1.0, 0.0]])[:ng]
    gate = _expand(pairs, keys).to(cuda)
    xd, Ad = x.to(cuda), A.to(cuda)
    with K.p8_tile_width(256):
        assert K.gemm_lora_tile(M, N, Kd, P, n_per, gr) == 256
        gated = K.linear_lora(xd, W.to(cuda), Ad, n_per, gr, b, residual=r, gate=gate, gate_div=div)
        variants = {}
        for pc, ps in {tuple(p) for p in pairs.tolist()}:
            Wv = W if pc else _zero_cols(W, Kd, keys, 0)
            Wv = Wv if ps else _zero_cols(Wv, Kd, keys, 1)
            variants[(pc, ps)] = K.linear_lora(xd, Wv.to(cuda), Ad, n_per, gr, b, residual=r)
        ones = K.linear_lora(xd, W.to(cuda), Ad, n_per, gr, b, residual=r, gate=torch.ones_like(gate), gate_div=div)
    assert not torch.equal(variants[(1.0, 1.0)], variants[(0.0, 0.0)])  # the delta is visible in the output
    if 1 in keys:
        assert not torch.equal(variants[(1.0, 0.0)], variants[(0.0, 1.0)])
    for i in range(ng):
        sl = slice(i * div, min((i + 1) * div, M))
        assert torch.equal(gated[sl], variants[tuple(pairs[i].tolist())][sl]), (i, pairs[i])
    assert torch.equal(ones, variants[(1.0, 1.0)])


@pytest.fixture(scope="module")
def persistent_case(cuda, K):
    M, Kd, n_per, r_per, P, div = 32768, 640, 640, 16, 32, 1024
    g = torch.Generator().manual_seed(M + 1)
    x, A, W = _operands(M, Kd, 1, n_per, r_per, P, g)
    b = torch.randn(n_per, generator=g) * 0.1
    r = rnd(M, n_per, gen=g)
    gate = torch.rand(M // div, P, generator=g) * 1.5 - 0.25
    return dict(x=x, A=A, W=W, b=b, r=r, gate=gate, div=div, n_per=n_per, r_per=r_per)


def test_gated_persistent_grid_bitwise_and_vs_fp32(cuda, K, persistent_case):
    """The persistent LoRA grid (128x320 tiles; the next tile's first k-tiles are in flight while lora_post reads the
    gate) with fractional gates: the bits of the one-workgroup-per-tile launch (VST_P8_LORA_PERSIST=0 in a child
    process, as test_gemm_lora_persistent_bitwise does it), and within test_gemm_lora_gpu's 5e-3 / 1e-2 of fp32 torch
    of the definition."""
    if os.environ.get("VST_P8_LORA_PERSIST", "1") != "1":
        pytest.skip("VST_P8_LORA_PERSIST is off in this process: both sides would run the one-tile-per-workgroup grid")
    c = persistent_case
    d = {k: v.to(cuda) for k, v in c.items() if torch.is_tensor(v)}
    M, Kd = c["x"].shape
    assert K.gemm_lora_tile(M, c["n_per"], Kd, 32, c["n_per"], c["r_per"]) == 320
    out = K.linear_lora(d["x"], d["W"], d["A"], c["n_per"], c["r_per"], d["b"], residual=d["r"], gate=d["gate"],
                        gate_div=c["div"])
    with tempfile.TemporaryDirectory() as tmp:
        torch.save({k: v for k, v in c.items() if torch.is_tensor(v)}, os.path.join(tmp, "in.pt"))
        code = (
            "import sys, torch; sys.path.insert(0, %r)\n"
            "from video_style_transfer_amd import kernels as K\n"
            "t = torch.load(%r, weights_only=True)\n"
            "c = {k: v.cuda() for k, v in t.items()}\n"
            "y = K.linear_lora(c['x'], c['W'], c['A'], %d, %d, c['b'], residual=c['r'], gate=c['gate'], gate_div=%d)\n"
            "torch.save(y.cpu(), %r)\n" % (ROOT, os.path.join(tmp, "in.pt"), c["n_per"], c["r_per"], c["div"],
                                             os.path.join(tmp, "out.pt")))
        subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VST_P8_LORA_PERSIST="0"), check=True,
                       timeout=240)
        ref = torch.load(os.path.join(tmp, "out.pt"), weights_only=True)
    assert torch.equal(out.cpu(), ref)
    # fp32 of the definition, on the device (the products are fp32 torch; only the two bf16 roundings of u are ours)
    xf, Wf = d["x"].float(), d["W"].float()
    u = (xf @ d["A"].float().t()).to(BF).float()
    u = (d["gate"].repeat_interleave(c["div"], 0) * u).to(BF).float()
    want = (xf @ Wf[:, :Kd].t() + u @ Wf[:, Kd:].t() + d["b"]).to(BF).float() + d["r"].float()
    check(out, want, 5e-3, 1e-2, "gated persistent 128x320 vs fp32")


# ----------------------------------------------------------------------------- vst_lora_gate
@pytest.mark.parametrize("P", [32, 64])
def test_lora_gate_kernel_equals_torch(cuda, K, P):
    M, div, ldu = 300, 77, P + 24
    g = torch.Generator().manual_seed(P)
    ubuf = rnd(M, ldu, gen=g)
    ng = (M + div - 1) // div
    gbuf = torch.randn(ng, P + 4, generator=g)
    gbuf[0, :4] = torch.tensor([0.0, 1.0, -2.5, 3.0])
    want = (gbuf[:, :P].repeat_interleave(div, 0)[:M] * ubuf[:, :P].float()).to(BF)
    ud, gd = ubuf.to(cuda), gbuf.to(cuda)
    u, gate = ud[:, :P], gd[:, :P]  # row strides ldu > P, ld_gate = P + 4
    out = K.lora_gate(u, gate, div)
    assert out.shape == (M, P) and torch.equal(out.cpu(), want)
    assert torch.equal(ud.cpu(), ubuf)  # out of place: u untouched
    ybuf = torch.zeros(M, P + 8, dtype=BF, device=cuda)
    assert K.lora_gate(u, gate, div, out=ybuf[:, :P]) is not None
    assert torch.equal(ybuf[:, :P].cpu(), want) and not ybuf[:, P:].any()
    r = K.lora_gate(u, gate, div, out=u)  # in place
    assert r.data_ptr() == u.data_ptr() and torch.equal(u.cpu(), want)
    assert torch.equal(ud[:, P:].cpu(), ubuf[:, P:])  # the columns past P are not touched
    from video_style_transfer_amd._lib import VstError
    with pytest.raises(VstError):
        K.lora_gate(u, gd[: ng - 1, :P], div)  # too few gate rows
    with pytest.raises(VstError):
        K.lora_gate(u, gd[:, 1:P + 1], div)  # misaligned gate base
    with pytest.raises(VstError):
        K.lora_gate(u, gate.double(), div)


def test_two_pass_with_lora_gate_matches_gated_gemm(cuda, K):
    """u from its own pass, vst_lora_gate, then the K-augmented GEMM, against the gated in-GEMM call on the same
    operands: test_gemm_lora_gpu's two-pass tolerance (an occasional 1-ulp difference of a bf16 u element)."""
    M, Kd, N, P, div = 600, 192, 192, 32, 100
    g = torch.Generator().manual_seed(21)
    x, A, W = _operands(M, Kd, 1, N, 16, P, g)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda)
    gate = (torch.rand((M + div - 1) // div, P, generator=g) * 2 - 0.5).to(cuda)
    xd, Ad, Wd = x.to(cuda), A.to(cuda), W.to(cuda)
    fused = K.linear_lora(xd, Wd, Ad, N, 16, b, gate=gate, gate_div=div)
    u = K.linear(xd, Ad, kind="gemm_lora_down")
    two = K.linear(xd, Wd, b, x2=K.lora_gate(u, gate, div))
    check(fused, two, 1e-3, 4e-3, "gated in-GEMM vs lora_gate + two-pass")
    assert not torch.equal(two, K.linear(xd, Wd, b, x2=u))  # the gate changes the output
    # run_ops takes the same two routes with a LoraGate (6 gate rows of 100 rows)
    from video_style_transfer_amd.lora_gate import LoraGate
    from video_style_transfer_amd.lora_linear import ProjOps, run_ops
    keys = (0,) * 8 + (1,) * 8 + (-1,) * 16
    lg = LoraGate(6, cuda).set(content=[1.0, 0.5, 0.0, 2.0, -1.0, 0.25], style=[0.0, 1.0, 0.75, 1.0, 3.0, 0.5])
    ops = ProjOps(Wd, Ad, b, Kd, N, 16, N, 16, keys)
    t = lg.expanded(keys)
    assert torch.equal(run_ops(xd, ops, gate=lg), K.linear_lora(xd, Wd, Ad, N, 16, b, gate=t, gate_div=100))
    assert torch.equal(run_ops(xd, ops, u=u.clone(), gate=lg), K.linear(xd, Wd, b, x2=K.lora_gate(u, t, 100)))


# ----------------------------------------------------------------------------- fused cross-attention
@pytest.fixture(scope="module")
def xattn_case(cuda):
    Nq, frames, N, Kd, Nk, P = 256, 4, 192, 128, 77, 32
    g = torch.Generator().manual_seed(31)
    x, A, W = _operands(frames * Nq, Kd, 1, N, 16, P, g)
    b = torch.randn(N, generator=g) * 0.1
    kv = (torch.randn(frames * Nk, 2 * N, generator=g) * 2.0).to(BF)
    keys = (0,) * 8 + (1,) * 8 + (-1,) * 16
    return dict(x=x, A=A, W=W, b=b, kv=kv, keys=keys, Nq=Nq, frames=frames, N=N, Kd=Kd, Nk=Nk, P=P)


def _xattn(K, c, cuda, W, gate=None):
    kv = c["kv"].to(cuda)
    return K.linear_cross_attention(c["x"].to(cuda), W.to(cuda), c["A"].to(cuda), c["N"], 16, c["b"].to(cuda),
                                    kv[:, :c["N"]], kv[:, c["N"]:], Nq=c["Nq"], Nk=c["Nk"], kv_div=1, scale=0.125,
                                    gate=gate, gate_div=c["Nq"])


def test_gated_cross_attention_binary_gates(cuda, K, xattn_case):
    """2 batch elements x 2 frames of 256 queries, 3 heads, one K/V block per frame (kv_div = 1), one gate row per
    frame: frame f equals, bit for bit, frame f of the ungated launch with the switched-off columns of V zeroed."""
    c = xattn_case
    M = c["frames"] * c["Nq"]
    assert K.cross_attention_fusable(M, c["N"], c["Kd"], True, c["P"], c["N"], 16, c["Nq"], c["Nk"])
    pairs = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]])
    K.profile_launches(True)
    gated = _xattn(K, c, cuda, c["W"], _expand(pairs, c["keys"]).to(cuda))
    rec = K.collect_launches()
    K.profile_launches(False)
    assert [r[1] for r in rec] == ["gemm_p8<256x192,lora,gate,xattn>"], rec
    outs = set()
    for f, (pc, ps) in enumerate(pairs.tolist()):
        Wv = c["W"] if pc else _zero_cols(c["W"], c["Kd"], c["keys"], 0)
        Wv = Wv if ps else _zero_cols(Wv, c["Kd"], c["keys"], 1)
        ref = _xattn(K, c, cuda, Wv)
        sl = slice(f * c["Nq"], (f + 1) * c["Nq"])
        assert torch.equal(gated[sl], ref[sl]), f
        outs.add(ref[:c["Nq"]].cpu().float().sum().item())
    assert len(outs) == 4  # the four V variants give four different outputs: the delta reaches the attention
    ones = _xattn(K, c, cuda, c["W"], torch.ones(c["frames"], c["P"], device=cuda))
    assert torch.equal(ones, _xattn(K, c, cuda, c["W"]))


def test_gated_cross_attention_vs_unfused(cuda, K, xattn_case):
    """Fractional gates: the fused launch against gated linear_lora -> spatial_attention, at test_gemm_xattn_gpu's
    fused-against-two-launch tolerance (2e-3 / 1e-2: one softmax pass against two online key tiles)."""
    c = xattn_case
    g = torch.Generator().manual_seed(32)
    gate = (torch.rand(c["frames"], c["P"], generator=g) * 2 - 0.5).to(cuda)
    fused = _xattn(K, c, cuda, c["W"], gate)
    kv = c["kv"].to(cuda)
    q = K.linear_lora(c["x"].to(cuda), c["W"].to(cuda), c["A"].to(cuda), c["N"], 16, c["b"].to(cuda), gate=gate,
                      gate_div=c["Nq"])
    two = K.spatial_attention(q, kv[:, :c["N"]], kv[:, c["N"]:], c["frames"], c["N"] // 64, c["Nq"], c["Nk"], 1,
                              scale=0.125)
    check(fused, two, 2e-3, 1e-2, "gated xattn fused vs two-launch")
    assert not torch.equal(fused, _xattn(K, c, cuda, c["W"]))


# ----------------------------------------------------------------------------- view contract
SENT = 0x7FA5  # a bf16 NaN pattern no kernel produces


def _nan_arena(t, dev, top=8, bottom=320, side=8):
    """t as the interior of a NaN-filled 2-D arena (row stride != cols, interior 16-byte aligned)."""
    rows, cols = t.shape
    ld = (side + cols + side + 7) // 8 * 8
    a = torch.full((top + rows + bottom, ld), float("nan"), dtype=t.dtype, device=dev)
    v = a[top:top + rows, side:side + cols]
    v.copy_(t)
    return v


def _out_arena(rows, cols, dev, top=8, bottom=320, side=8):
    ld = (side + cols + side + 7) // 8 * 8
    a = torch.empty((top + rows + bottom, ld), dtype=BF, device=dev)
    a.view(torch.int16).fill_(SENT)
    return a[top:top + rows, side:side + cols], a, (top, side)


def _verify_arena(name, full, origin, rows, cols):
    same = full.view(torch.int16) == SENT
    outside = ~same
    outside[origin[0]:origin[0] + rows, origin[1]:origin[1] + cols] = False
    assert not outside.any(), f"{name}: written outside the view at {outside.nonzero()[:4].tolist()}"
    inner = full[origin[0]:origin[0] + rows, origin[1]:origin[1] + cols]
    assert not same[origin[0]:origin[0] + rows, origin[1]:origin[1] + cols].any(), f"{name}: unwritten elements"
    assert torch.isfinite(inner.float()).all(), f"{name}: non-finite values leaked in"


def _gate_arena(gate, dev, extra_rows=3):
    """The gate inside NaN: padding columns (ld_gate = P + 8 > P) and rows past ng are NaN; 16-byte aligned base."""
    ng, P = gate.shape
    a = torch.full((ng + extra_rows, P + 8), float("nan"), dtype=torch.float32, device=dev)
    a[:ng, :P] = gate
    v = a[:ng, :P]
    assert v.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("bn,N", [(192, 192), (256, 192), (320, 320)])
def test_view_contract_gated_gemm(cuda, K, bn, N):
    """Operands and output are views inside NaN / sentinel guard bands, the gate table has NaN in its padding columns
    and in rows past ceil(M / gate_div): the output is finite, equals the call on plain tensors, and nothing outside
    it is written (M = 300: the tail tile's rows >= M must not fetch a gate row past the table)."""
    M, Kd, P, div = 300, 136, 32, 77
    g = torch.Generator().manual_seed(bn)
    x, A, W = _operands(M, Kd, 1, N, 16, P, g)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda)
    r = rnd(M, N, gen=g)
    gate = torch.rand((M + div - 1) // div, P, generator=g) + 0.5
    with K.p8_tile_width(bn):
        assert K.gemm_lora_tile(M, N, Kd, P, N, 16) == bn
        ref = K.linear_lora(x.to(cuda), W.to(cuda), A.to(cuda), N, 16, b, residual=r.to(cuda), gate=gate.to(cuda),
                            gate_div=div)
        out, full, org = _out_arena(M, N, cuda)
        K.linear_lora(_nan_arena(x, cuda), _nan_arena(W, cuda), _nan_arena(A, cuda), N, 16, b,
                      residual=_nan_arena(r, cuda), out=out, gate=_gate_arena(gate, cuda), gate_div=div)
    _verify_arena(f"gated gemm {bn}", full, org, M, N)
    assert torch.equal(out, ref)


def test_view_contract_gated_cross_attention_and_lora_gate(cuda, K, xattn_case):
    c = xattn_case
    M = c["frames"] * c["Nq"]
    g = torch.Generator().manual_seed(41)
    gate = torch.rand(c["frames"], c["P"], generator=g) + 0.5
    ref = _xattn(K, c, cuda, c["W"], gate.to(cuda))
    out, full, org = _out_arena(M, c["N"], cuda)
    kv = _nan_arena(c["kv"], cuda)
    K.linear_cross_attention(_nan_arena(c["x"], cuda), _nan_arena(c["W"], cuda), _nan_arena(c["A"], cuda), c["N"], 16,
                             c["b"].to(cuda), kv[:, :c["N"]], kv[:, c["N"]:], Nq=c["Nq"], Nk=c["Nk"], kv_div=1,
                             scale=0.125, out=out, gate=_gate_arena(gate, cuda), gate_div=c["Nq"])
    _verify_arena("gated xattn", full, org, M, c["N"])
    assert torch.equal(out, ref)
    # vst_lora_gate, out of place and in place, on views
    Mu, P, div = 300, 32, 77
    u = rnd(Mu, P, gen=g)
    gt = torch.randn((Mu + div - 1) // div, P, generator=g)
    want = (gt.repeat_interleave(div, 0)[:Mu] * u.float()).to(BF)
    y, yfull, yorg = _out_arena(Mu, P, cuda)
    K.lora_gate(_nan_arena(u, cuda), _gate_arena(gt, cuda), div, out=y)
    _verify_arena("lora_gate", yfull, yorg, Mu, P)
    assert torch.equal(y.cpu(), want)
    y2, y2full, y2org = _out_arena(Mu, P, cuda)
    y2.copy_(u)
    K.lora_gate(y2, _gate_arena(gt, cuda), div, out=y2)
    _verify_arena("lora_gate in place", y2full, y2org, Mu, P)
    assert torch.equal(y2.cpu(), want)


# ----------------------------------------------------------------------------- the attention processor
def _attention(cuda, cross_dim, seed):
    from video_style_transfer_amd.attention_processor import Attention
    from video_style_transfer_amd.utils import attach_unziplora_layers
    torch.manual_seed(seed)
    attn = Attention(128, cross_dim, 2, 64)
    holder = torch.nn.Module()
    holder.blk = torch.nn.Module()
    setattr(holder.blk, "attn2" if cross_dim else "attn1", attn)  # the module-name pattern the attach helper matches
    attach_unziplora_layers(holder, 8)
    holder.to(cuda).requires_grad_(False)
    with torch.no_grad():
        for name, p in holder.named_parameters():
            if "lora" in name and "up" in name:
                p.normal_(0.0, 0.2)
    return attn


@pytest.mark.parametrize("cross", [False, True])
def test_processor_per_frame_gates_equal_uniform_runs(cuda, K, cross):
    """B = 2 clips x F = 3 frames of 256 tokens, C = 128, a different (content, style) pair per frame.  Without
    cross-frame attention the frames are independent, so frame f of the gated batch is, bit for bit, frame f of a
    run that uses f's pair for every frame.  attn1 takes the explicit-u route for q/k/v (vst_lora_gate) and the
    in-GEMM gate for to_out; attn2 the fused gated cross-attention launch, with per-frame text K/V.  Run as the
    UNet runs it, under K.row_invariant (a row's bits do not depend on the launch's row count: the gated text K/V
    are projected for 6 x 77 rows, the plain ones for 2 x 77)."""
    from video_style_transfer_amd.attention_processor import AnimateDiffAttnProcessor2_0, AttnCall
    from video_style_transfer_amd.lora_gate import LoraGate
    attn = _attention(cuda, 128 if cross else None, 5 + cross)
    proc = AnimateDiffAttnProcessor2_0()
    g = torch.Generator().manual_seed(6)
    x = rnd(6, 256, 128, scale=0.5, gen=g).to(cuda)
    res = rnd(6, 256, 128, gen=g).to(cuda)
    enc = rnd(2, 77, 128, gen=g).to(cuda) if cross else None
    pairs = torch.tensor([[1.0, 1.0], [0.5, 1.0], [1.0, 0.0], [0.0, 0.0], [1.5, -0.5], [0.25, 0.75]])
    gate = LoraGate(6, cuda).set(pairs[:, 0], pairs[:, 1])
    K.profile_launches(True)
    with K.row_invariant():
        out = proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(residual=res, lora_gate=gate))
    rec = K.collect_launches()
    K.profile_launches(False)
    syms = [r[1] for r in rec]
    assert any(s and s.startswith("gemm_p8<") and ",lora,gate>" in s for s in syms), syms  # to_out, in-GEMM
    if cross:
        assert "gemm_p8<256x192,lora,gate,xattn>" in syms, syms
    else:
        assert "lora_gate" in [r[0] for r in rec], rec
    with K.row_invariant():
        plain = proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(residual=res))
        assert not torch.equal(out, plain) and torch.equal(out[0], plain[0])  # frame 0 has gates (1, 1)
        for f in range(6):
            uni = LoraGate(6, cuda).set(float(pairs[f, 0]), float(pairs[f, 1]))
            ref = proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(residual=res, lora_gate=uni))
            assert torch.equal(out[f], ref[f]), f
    from video_style_transfer_amd._lib import VstError
    with pytest.raises(VstError):
        proc(attn, x, encoder_hidden_states=enc, _vst=AttnCall(residual=res, lora_gate=LoraGate(4, cuda)))


def test_text_kv_reprojects_in_place_when_gates_change(cuda, K):
    from video_style_transfer_amd.attention_processor import _text_kv, refresh_text_kv
    from video_style_transfer_amd.lora_gate import LoraGate
    attn = _attention(cuda, 128, 8)
    enc = rnd(2, 77, 128, gen=torch.Generator().manual_seed(9)).to(cuda)
    gate = LoraGate(6, cuda).set(1.0, torch.linspace(0, 1, 6))
    with K.row_invariant():
        kv = _text_kv(attn, enc, 1.0, gate)
        assert kv.shape == (6 * 77, 256)
        assert _text_kv(attn, enc, 1.0, gate) is kv
        old = kv.clone()
        ungated = _text_kv(attn, enc, 1.0)
    assert ungated.shape == (2 * 77, 256)
    assert torch.equal(old[5 * 77:], ungated[77:])  # the frame with gates (1, 1) is the plain projection
    gate.set(1.0, 0.0)
    refresh_text_kv(attn, gate)
    assert not torch.equal(kv, old)  # the same buffer, new values
    with K.row_invariant():
        fresh = _text_kv(attn, enc, 1.0, LoraGate(6, cuda).set(1.0, 0.0))
        assert fresh.data_ptr() != kv.data_ptr() and torch.equal(fresh, kv)
        gate.set(1.0, torch.linspace(0, 1, 6))
        assert _text_kv(attn, enc, 1.0, gate) is kv and torch.equal(kv, old)  # the lookup refreshes a stale entry too


# ----------------------------------------------------------------------------- the UNet against fp32
F_U, HW_U = 3, 32


@pytest.fixture(scope="module")
def unet_case(cuda):
    """Tiny config, B = 2 clips of F = 3 frames at 32x32 latents (the 16x16 level fuses attn2), the HIP model, its
    ungated output and the fp32 oracle of the ungated forward -- computed once for the tests below."""
    from oracle.unet import unet_forward
    from test_parity_gpu import _setup, rel
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", F_U, HW_U, seed=3, B=2)
    t = torch.tensor([501.0, 501.0])
    unet = build_unet(cfg, state_dict=sd, device=cuda)

    def run(model=unet, **kw):
        return model(lat.to(cuda), t.to(cuda), enc.to(cuda),
                     added_cond_kwargs={"text_embeds": pooled.to(cuda), "time_ids": tids.to(cuda)}, **kw).sample

    plain = run()
    ref = unet_forward(sd, cfg.to_dict(), lat, t, enc, pooled, tids)
    base = rel(plain, ref)
    print(f"[gate] ungated UNet vs oracle: rel_l2={base[0]:.3e} rel_max={base[1]:.3e}")
    return dict(cfg=cfg, sd=sd, lat=lat, enc=enc, pooled=pooled, tids=tids, t=t, unet=unet, run=run, plain=plain,
                ref=ref, base=base)


def _gate_for(case, cuda, content, style):
    """LoraGate over the B * F rows from per-clip [B] or per-frame [B, F] values (or scalars)."""
    from video_style_transfer_amd.lora_gate import LoraGate

    def rows(v):
        v = torch.as_tensor(v, dtype=torch.float32)
        if v.dim() == 0:
            return v.expand(2 * F_U)
        return (v[:, None].expand(2, F_U) if v.dim() == 1 else v).reshape(-1)
    return LoraGate(2 * F_U, cuda).set(rows(content), rows(style))


def _assert_within_ungated_error(case, out, ref, name):
    """At most 1.5x the ungated forward's rel-L2 and rel-max against the oracle, measured on the same inputs."""
    from test_parity_gpu import rel
    e2, em = rel(out, ref)
    b2, bm = case["base"]
    print(f"[gate] {name}: rel_l2={e2:.3e} ({e2 / b2:.2f}x ungated {b2:.3e}) rel_max={em:.3e} "
          f"({em / bm:.2f}x ungated {bm:.3e})")
    assert e2 <= 1.5 * b2 and em <= 1.5 * bm, (name, e2, b2, em, bm)


def _scaled_up_factors(sd, gc, gs):
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith("content_up.weight"):
            out[k] = v * gc
        elif k.endswith("style_up.weight"):
            out[k] = v * gs
    return out


@pytest.mark.parametrize("content,style", [(0.7, 0.6), ([1.0, 0.4], [0.3, 1.2])], ids=["uniform", "per_clip"])
def test_unet_uniform_and_per_clip_gates_vs_oracle(cuda, unet_case, content, style):
    """The reference is oracle.unet.unet_forward on a state dict whose content_up / style_up weights are multiplied
    by the gates, one batch element at a time (a gate on u's columns scales the term as a scale on the up factor
    does)."""
    from oracle.unet import unet_forward
    c = unet_case
    out = c["run"](lora_gate=_gate_for(c, cuda, content, style))
    gc = torch.as_tensor(content, dtype=torch.float32).expand(2)
    gs = torch.as_tensor(style, dtype=torch.float32).expand(2)
    refs = []
    for b in range(2):
        sdb = _scaled_up_factors(c["sd"], float(gc[b]), float(gs[b]))
        refs.append(unet_forward(sdb, c["cfg"].to_dict(), c["lat"][b:b + 1], c["t"][b:b + 1], c["enc"][b:b + 1],
                                 c["pooled"][b:b + 1], c["tids"][b:b + 1]))
    ref = torch.cat(refs)
    assert not torch.equal(out, c["plain"])
    _assert_within_ungated_error(c, out, ref, f"UNet gates content={content} style={style}")


def test_unet_per_frame_gates_vs_oracle(cuda, unet_case, monkeypatch):
    """Per-frame gates with the motion modules on.  The reference is unet_forward with oracle.unet.proj wrapped for
    this test: the content and the style delta from two unziplora_delta calls with the other key masked, each
    scaled by the gate of its leading-dimension row (spatial states and the repeated text states are [B * F, ...];
    the motion modules' projections carry no UnZipLoRA and pass through)."""
    import oracle.unet as OU
    from oracle.ref_ops import lora_compatible_linear, unziplora_delta
    c = unet_case
    g = torch.Generator().manual_seed(12)
    gc = torch.rand(2, F_U, generator=g) * 1.5
    gs = torch.linspace(0.0, 1.0, F_U).expand(2, F_U).clone()
    gs[1] = gs[1].flip(0) * 1.25
    orig = OU.proj

    def gated_proj(P, name, x, lora):
        lk = name + ".lora_layer.lora_matrix_dic.content_down.weight"
        if lora is None or lk not in P:
            return orig(P, name, x, lora)
        assert x.shape[0] == 2 * F_U, (name, x.shape)
        pre = name + ".lora_layer."
        args = (P[pre + "lora_matrix_dic.content_down.weight"], P[pre + "lora_matrix_dic.content_up.weight"],
                P[pre + "merge_content"], P[pre + "lora_matrix_dic.style_down.weight"],
                P[pre + "lora_matrix_dic.style_up.weight"], P[pre + "merge_style"], lora.forward_type)
        dc = unziplora_delta(x, *args, False, True)
        ds = unziplora_delta(x, *args, True, False)
        shape = (-1,) + (1,) * (x.dim() - 1)
        delta = gc.reshape(shape) * dc + gs.reshape(shape) * ds
        b = OU._p(P, name + ".bias") if name + ".bias" in P else None
        return lora_compatible_linear(x, OU._p(P, name + ".weight"), b, delta, lora.scale)

    monkeypatch.setattr(OU, "proj", gated_proj)
    ref = OU.unet_forward(c["sd"], c["cfg"].to_dict(), c["lat"], c["t"], c["enc"], c["pooled"], c["tids"])
    monkeypatch.undo()
    assert c["cfg"].motion_modules and not torch.equal(ref, c["ref"])
    out = c["run"](lora_gate=_gate_for(c, cuda, gc, gs))
    _assert_within_ungated_error(c, out, ref, "UNet per-frame gates")


def test_unet_gates_one_and_zero_are_exact(cuda, unet_case):
    """Gates of 1 are the ungated forward bit for bit; gates of 0 are the forward of the same model with every LoRA
    up factor zeroed (a zero u column and a zero V column add the same exact zeros)."""
    from video_style_transfer_amd.utils import build_unet
    c = unet_case
    assert torch.equal(c["run"](lora_gate=_gate_for(c, cuda, 1.0, 1.0)), c["plain"])
    zero = build_unet(c["cfg"], state_dict=_scaled_up_factors(c["sd"], 0.0, 0.0), device=cuda)
    want = c["run"](model=zero)
    assert not torch.equal(want, c["plain"])
    assert torch.equal(c["run"](lora_gate=_gate_for(c, cuda, 0.0, 0.0)), want)
    from video_style_transfer_amd._lib import VstError
    from video_style_transfer_amd.lora_gate import LoraGate
    with pytest.raises(VstError):
        c["run"](lora_gate=LoraGate(5, cuda))  # rows != B * F


# ----------------------------------------------------------------------------- the denoiser
N_STEPS, GUIDANCE = 10, 7.5


@pytest.fixture(scope="module")
def tiny(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 4, 16, seed=5, B=2)
    g = torch.Generator().manual_seed(77)
    z0 = torch.randn(1, 4, 4, 16, 16, generator=g)
    mask = (torch.rand(1, 4, 16, 16, generator=g) < 0.5).float()
    return dict(enc=enc, pooled=pooled, unet=build_unet(cfg, state_dict=sd, device=cuda), z0=z0, mask=mask)


def _denoiser(tiny, cuda, use_graph=True, frames=4, **kw):
    from video_style_transfer_amd.pipeline import AnimateDiffDenoiser
    den = AnimateDiffDenoiser(tiny["unet"], frames, 128, 128, num_inference_steps=N_STEPS, guidance_scale=GUIDANCE,
                              device=cuda, use_graph=use_graph, **kw)
    den.set_prompt_embeds(tiny["enc"][1:2], tiny["pooled"][1:2], tiny["enc"][0:1], tiny["pooled"][0:1])
    return den


RAMP = torch.linspace(0.0, 1.0, 4)


def test_denoiser_graph_equals_eager_and_new_values_keep_the_graph(cuda, tiny):
    dg, de = _denoiser(tiny, cuda, True), _denoiser(tiny, cuda, False)
    plain = _denoiser(tiny, cuda)(seed=3).clone()
    og = dg(seed=3, style_scale=RAMP).clone()
    oe = de(seed=3, style_scale=RAMP).clone()
    assert dg.graph is not None and de.graph is None
    assert torch.isfinite(og).all() and torch.equal(og, oe) and not torch.equal(og, plain)
    # new values after capture: the same graph object and gate buffers, the bits of a fresh eager denoiser given
    # those gates (stale text K/V in the captured buffers would show here)
    g0, gate = dg.graph, dg.lora_gate
    ptrs = [t.data_ptr() for _, t in gate._expanded.values()]
    new_c, new_s = torch.tensor([1.0, 0.5, 1.5, 0.0]), RAMP.flip(0) * 1.2
    dg.set_lora_gates(new_c, new_s)
    og2 = dg(seed=3).clone()
    assert dg.graph is g0 and dg.lora_gate is gate
    assert ptrs == [t.data_ptr() for _, t in gate._expanded.values()]
    fresh = _denoiser(tiny, cuda, False)
    assert torch.equal(og2, fresh(seed=3, content_scale=new_c, style_scale=new_s))
    assert not torch.equal(og2, og)
    # a schedule from the host: the gates change between two replays of the same captured step
    dg.set_lora_gates(style=RAMP)
    dg.init_latents(3)
    dg.run_steps(4)
    dg.set_lora_gates(new_c, new_s)
    sched = dg.run_steps(N_STEPS - 4).clone()
    assert dg.graph is g0
    de.set_lora_gates(style=RAMP)
    de.init_latents(3)
    de.run_steps(4)
    de.set_lora_gates(new_c, new_s)
    assert torch.equal(sched, de.run_steps(N_STEPS - 4))
    # gates of 1 are the plain run; clearing drops the captured step and gives the plain run again
    dg.set_lora_gates(1.0, 1.0)
    assert torch.equal(dg(seed=3), plain) and dg.graph is g0
    dg.clear_lora_gates()
    assert dg.graph is None and dg.lora_gate is None
    assert torch.equal(dg(seed=3), plain)


def test_denoiser_first_set_drops_a_captured_plain_step(cuda, tiny):
    den = _denoiser(tiny, cuda)
    plain = den(seed=3).clone()
    assert den.graph is not None
    den.set_lora_gates(style=RAMP)
    assert den.graph is None
    gated = den(seed=3).clone()
    assert den.graph is not None and not torch.equal(gated, plain)
    eager = _denoiser(tiny, cuda, False)
    assert torch.equal(gated, eager(seed=3, style_scale=RAMP))


@pytest.mark.parametrize("what", ["source_mask", "cross_frame"])
def test_denoiser_gates_compose_graph_equals_eager(cuda, tiny, what):
    outs = []
    for use_graph in (True, False):
        if what == "source_mask":
            den = _denoiser(tiny, cuda, use_graph)
            outs.append(den(source=tiny["z0"], strength=0.3, mask=tiny["mask"], seed=42, content_scale=0.8,
                            style_scale=RAMP).clone())
        else:
            den = _denoiser(tiny, cuda, use_graph, cross_frame=("first",))
            outs.append(den(seed=3, style_scale=RAMP).clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_denoiser_gates_compose_with_long_clip(cuda):
    from test_parity_gpu import _setup
    from video_style_transfer_amd.utils import build_unet
    cfg, sd, lat, enc, pooled, tids = _setup("tiny", 20, 16)
    t20 = dict(unet=build_unet(cfg, state_dict=sd, device=cuda), enc=enc, pooled=pooled)
    ramp = torch.linspace(0.0, 1.0, 20)
    outs = []
    for use_graph in (True, False):
        den = _denoiser(t20, cuda, use_graph, frames=20, context_length=16, context_stride=4)
        outs.append(den(seed=3, style_scale=ramp).clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
