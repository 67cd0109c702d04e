"""Float64 reference, derived per-element bound, input families, shape
generator and an fp32 emulation for the grouped GEMM (include/s3n.h s3n_gemm,
csrc/net_gemm*.hip), for tests/test_gemm.py.

Plain PyTorch, device agnostic: the oracle tests run it on the CPU, the GPU
tests on the device, where the reference of one (shape, family) is computed
once and shared by both layouts and both output types.  Nothing of the
kernels' tiling appears in `reference`: it restates s3n.h lines 39-49 in
float64 from the fp16 / fp32 input bits,

    lin = A B^T (or the conv of the NHWC image, ReLU on the image first)
    x   = lin + bias, RoPE2D on the first rope_ncols columns
    y   = act(x) + R1 + R2            (GELU with the exact erf)
    tail_out = y tail_w^T + tail_b

Bound, per output element, from the arithmetic and not from measured results,
with u = 2^-24 (fp32 unit roundoff) and S = |A| |B|^T:

  * accumulation: e_acc = K u_acc S, the first-order bound of K fp32 additions
    of exact fp16 products in any order, so it holds for every tile, K-group
    count and split-K.  u_acc = 2^-23: whether the MFMA's internal additions
    round to nearest is not documented, and 2^-23 covers truncation too.
    The bias add contributes u |x|:              e(x) = e_acc + u |x|.
  * RoPE: x c -+ x' s with fp32 tables read from the same bits in the
    reference: e = e(x) + e(x') + 2 u (|x c| + |x' s|).
  * activation: ReLU and none have slope <= 1 and are exact: e stays.  GELU
    has slope <= 1.13; the kernels' erf (Abramowitz & Stegun 7.1.26 on the
    hardware rcp / exp2) is within 4.7e-7 absolute (erf_fast's comment,
    test_net_ops.py test_gemm_gelu_erf_accuracy), which moves the result by
    0.5 |x| 4.7e-7; the three fp32 operations around it give 3 u |gelu(x)|:
        e(a) = 1.13 e(x) + 0.5 |x| 4.7e-7 + 3 u |gelu(x)|.
  * each residual add: u |partial sum|; an fp16 residual converts exactly.
  * fp16 store: 2^-11 |ref|.  C2 is the same fp32 value rounded the same
    way, so C2 == C.half() bit for bit whenever both exist.
  * fused tail (net_gemm_kernel.hpp epilogue_vec): the finished fp32 row y,
    residuals included, times fp16 weights, accumulated in fp32 over the N
    columns: |tail_w| e(y) + N u (|y| |tail_w|^T) + u |out|.

The worst-case e_acc grows like K^1.5 on random data, so at long K the bound
carries only the gross-error check (per element, where the older tests
normalise by the global maximum) and the rounding checks live at short K:
test_gemm.py::test_oracle_bound_sees_planted_defects plants an accumulator
rounded to fp16, a tanh GELU and a dropped k term and finds the largest K of
the generator's list at which each still exceeds twice the bound.  Addressing
at every K is carried by the families `exact` and `onehot_k`, whose outputs
are exact in fp32 and fp16 in any summation order and are compared without
any tolerance.

Families (all seeded, every group its own data):
  random    A ~ N(0,1), B ~ N(0,1/K), bias, R1, R2 ~ N(0,1); with the bound.
  exact     A, B in {-1,0,1}, bias and residuals integers in [-8,8], act none
            or ReLU: with K <= 1024 every partial sum is an integer below
            2048; equality with the reference.
  onehot_k  row i of A is 2^(i % 5 - 2) at k = pi(i) and zero elsewhere, B
            full-mantissa fp16: every element is one exact product (rounded
            once for an fp16 output; |B| >= 2^-8 keeps the products in fp16's
            normal range); pi visits 0, K-1 and both sides of every
            multiple of 8 (so of 32, the K tile, the K-group stride and the
            split boundaries, which come first in the list).
  onehot_conv  one non-zero pixel and channel per image: every output pixel is
            one weight (times a power of two) or zero.
A `cancel` family (lin == 0 by construction, S large) was considered and
left out: its check is `err <= tol` with the same bound as `random`, and the
epilogue-only error it would isolate is what `exact` already pins bit for bit.

Layouts: `dense` (every ld equals its extent) and `padded` (lda = K + 24,
ldb = K + 8, ldc = N + 16, ldr1 = N + 8, ldr2 = N + 24, ldc2 = N + 40), both
with 8 spare rows behind every operand; input padding and spare rows (and 8
elements behind the bias) are NaN, outputs are pre-filled with a NaN sentinel
(fp16 0x7E5A, fp32 0x7FC5A5A5), so a read shows in the result and a store
outside M x N shows in the footprint check.
"""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

import attention_ref64 as AR

U = 2.0 ** -24
U_ACC = 2.0 ** -23
ERF_ERR = 4.7e-7
GELU_SLOPE = 1.13
SENTINEL16 = 0x7E5A
SENTINEL32 = 0x7FC5A5A5
SPARE = 8                 # spare rows behind every operand
WS_SPARE = 64             # sentinel floats behind the split-K workspace
FAMILIES = ("random", "exact", "onehot_k")
PAD = dict(lda=24, ldb=8, ldc=16, ldr1=8, ldr2=24, ldc2=40, ld_tail=8)


# --------------------------------------------------------------- reference ---
def _act64(x, act):
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))
    if act == "relu":
        return x.clamp_min(0)
    assert act == "none", act
    return x


def conv_geometry(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _lin64(A, B, conv, absolute=False):
    """A [M,K] fp16 (or the NHWC image [Bn,H,W,Cin] with conv = dict(k, stride,
    pad, relu_in)), B [N,K] -> lin (or S with absolute) [M,N] float64."""
    a, b = A.double(), B.double()
    if conv is None:
        if absolute:
            a, b = a.abs(), b.abs()
        return a @ b.T
    if conv.get("relu_in"):
        a = a.clamp_min(0)
    if absolute:
        a, b = a.abs(), b.abs()
    k, cin = conv["k"], A.shape[-1]
    w = b.reshape(-1, k, k, cin).permute(0, 3, 1, 2)          # [Cout, Cin, ky, kx]
    o = F.conv2d(a.permute(0, 3, 1, 2), w, stride=conv["stride"], padding=conv["pad"])
    return o.permute(0, 2, 3, 1).reshape(-1, B.shape[0])


def _rope_cols(x, rope, mode):
    """RoPE2D on the first ncols columns of x [M, N]; rope = (pos [M,2], cos,
    sin, ncols).  'value' rotates (attention_ref64.rope64 on [1,H,M,64]), 'err'
    maps an error e to e(x) + e(x') and 'mag' gives |x c| + |x' s|, x' being
    the partner column j ^ 16 of the same half of a 64-wide head."""
    pos, cos, sin, ncols = rope
    if ncols == 0:
        return x if mode != "mag" else torch.zeros_like(x)
    M = x.shape[0]
    out = x.clone() if mode != "mag" else torch.zeros_like(x)
    if mode == "value":
        xh = x[:, :ncols].reshape(1, M, ncols // 64, 64).permute(0, 2, 1, 3)
        r = AR.rope64(xh, pos[None], cos, sin)
        out[:, :ncols] = r.permute(0, 2, 1, 3).reshape(M, ncols)
        return out
    j = torch.arange(ncols, device=x.device)
    xp = x[:, j ^ 16]
    if mode == "err":
        out[:, :ncols] = x[:, :ncols] + xp
        return out
    p = pos[:, (j % 64) // 32]                        # [M, ncols]: y for dims < 32, x above
    c, s = cos.double()[p, j % 16], sin.double()[p, j % 16]
    out[:, :ncols] = (x[:, :ncols] * c).abs() + (xp * s).abs()
    return out


def terms(A, B, bias=None, act="none", R1=None, R2=None, conv=None, rope=None, tail=None):
    """The reference and every magnitude the bound needs.  R1 / R2 [M,N] of
    any float type, rope = (pos [M,2] int64, cos, sin, ncols), tail =
    (tail_w [tail_n, N] fp16, tail_b [tail_n] fp32 or None)."""
    t = types.SimpleNamespace()
    t.K = B.shape[1]
    t.lin = _lin64(A, B, conv)
    t.S = _lin64(A, B, conv, absolute=True)
    x = t.lin if bias is None else t.lin + bias.double()
    e = t.K * U_ACC * t.S
    if bias is not None:
        e = e + U * x.abs()
    if rope is not None:
        e = _rope_cols(e, rope, "err") + 2 * U * _rope_cols(x, rope, "mag")
        x = _rope_cols(x, rope, "value")
    y = _act64(x, act)
    if act == "gelu":
        e = GELU_SLOPE * e + 0.5 * x.abs() * ERF_ERR + 3 * U * y.abs()
    for R in (R1, R2):
        if R is not None:
            y = y + R.double()
            e = e + U * y.abs()
    t.x, t.y, t.e = x, y, e
    if tail is not None:
        tw, tb = tail[0].double(), tail[1]
        t.tail = y @ tw.T + (0 if tb is None else tb.double())
        t.tail_e = (e @ tw.abs().T + y.shape[1] * U * (y.abs() @ tw.abs().T) + U * t.tail.abs())
    return t


def reference(A, B, **kw):
    """The pre-rounding value in the plain [M, N] layout, float64."""
    return terms(A, B, **kw).y


def tolerance(t, f16_out):
    """The bound of the module docstring for the output of terms()."""
    return t.e + (2.0 ** -11 * t.y.abs() if f16_out else 0)


def scatter(ref, mode, sH, sW, s, Cout):
    """[M, N] -> NHWC [B, sH*s, sW*s, Cout] by the index formulas of s3n.h:
    convt n = (i*s + j)*Cout + co, pixshuf n = co*s*s + i*s + j."""
    Bn = ref.shape[0] // (sH * sW)
    if mode == "convt":
        r = ref.reshape(Bn, sH, sW, s, s, Cout).permute(0, 1, 3, 2, 4, 5)
    else:
        assert mode == "pixshuf", mode
        r = ref.reshape(Bn, sH, sW, Cout, s, s).permute(0, 1, 4, 2, 5, 3)
    return r.reshape(Bn, sH * s, sW * s, Cout)


def worst(o, ref, tol):
    """Worst err / tol and its index; a NaN anywhere counts as infinite."""
    ratio = (o.double() - ref).abs() / tol
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    flat = int(ratio.argmax())
    return float(ratio.reshape(-1)[flat]), tuple(int(i) for i in np.unravel_index(flat, ratio.shape))


# ---------------------------------------------------------------- families ---
def onehot_positions(K, bk, kg, splits=(1, 2, 3)):
    """k positions pi visits, most telling first: 0, K-1, both sides of every
    split boundary, K-group stride, K tile, then of every multiple of 32 and
    8."""
    kt = -(-K // bk)
    edges = []
    for s in splits:
        per = -(-kt // s)
        edges += [per * bk * i for i in range(1, s + 1)]
    for step in (kg * bk, bk, 32, 8):
        edges += list(range(step, K, step))
    out = [0, K - 1]
    for e in edges:
        if 0 < e < K:
            out += [e - 1, e]
    return list(dict.fromkeys(out))


def onehot_pixels(H, W, C):
    """(y, x, c) the non-zero pixel visits: the four corners, the first and
    last column of every row, each with the last channel and channel 0."""
    px = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for y in range(H):
        px += [(y, 0), (y, W - 1)]
    px = list(dict.fromkeys(px))
    return [(y, x, C - 1 if i % 2 == 0 else 0) for i, (y, x) in enumerate(px)]


def _normal_range(b):
    """Full-mantissa values with |b| >= 2^-8: times 2^-2 they stay in fp16's
    normal range (the one-hot families pin addressing, not subnormals)."""
    return torch.where(b < 0, b.clamp_max(-2.0 ** -8), b.clamp_min(2.0 ** -8))


def make_data(family, M, N, K, groups, seed=0, device="cpu", conv=None, tile=(64, 1)):
    """Compact per-group values dict(A, B, bias, R1, R2): A [M,K] fp16 (conv =
    dict(Bn, H, W, C, k, stride, pad): the NHWC image), B [N,K] fp16, bias [N]
    fp32, R1 [M,N] fp32, R2 [M,N] fp16.  tile = (bk, kg) orders onehot_k."""
    assert family in FAMILIES + ("onehot_conv",), family
    out = []
    ashape = (M, K) if conv is None else (conv["Bn"], conv["H"], conv["W"], conv["C"])
    for g in range(groups):
        gen = torch.Generator(device=device)
        gen.manual_seed(1000003 * seed + 7919 * g + len(family))
        rn = lambda *s: torch.randn(*s, generator=gen, device=device)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen, device=device).float()
        if family == "exact":
            d = dict(A=ri(-1, 1, *ashape), B=ri(-1, 1, N, K), bias=ri(-8, 8, N),
                     R1=ri(-8, 8, M, N), R2=ri(-8, 8, M, N))
        else:
            d = dict(A=rn(*ashape), B=rn(N, K) * K ** -0.5, bias=rn(N), R1=rn(M, N), R2=rn(M, N))
        if family == "onehot_k":
            sp = onehot_positions(K, *tile)
            i = torch.arange(M, device=device)
            pi = torch.tensor([sp[(g * M + r) % len(sp)] for r in range(M)], device=device)
            d["A"] = torch.zeros(M, K, device=device)
            d["A"][i, pi] = 2.0 ** (i % 5 - 2).float()
            d["B"] = _normal_range(rn(N, K))
            d["pi"] = pi
        if family == "onehot_conv":
            sp = onehot_pixels(conv["H"], conv["W"], conv["C"])
            d["A"] = torch.zeros(*ashape, device=device)
            d["px"] = []
            for b in range(conv["Bn"]):
                y, x, c = sp[(seed + g * conv["Bn"] + b) % len(sp)]
                d["A"][b, y, x, c] = 2.0 ** ((g + b) % 5 - 2)
                d["px"].append((y, x, c))
            d["B"] = _normal_range(rn(N, K))
        d["A"], d["B"], d["R2"] = d["A"].half(), d["B"].half(), d["R2"].half()
        out.append(d)
    return out


def _pad2(x, ld, fill=math.nan):
    """x [r, c] inside a [r + SPARE, ld] allocation of `fill`; returns the
    allocation (the operand pointer is its base)."""
    buf = torch.full((x.shape[0] + SPARE, ld), fill, dtype=x.dtype, device=x.device)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf


def embed(data, layout, b_rows_only=False):
    """Per-group operands inside NaN-padded allocations.  b_rows_only: B keeps
    ldb == K (the B-direct tiles' packed copy is built only then)."""
    assert layout in ("dense", "padded"), layout
    p = PAD if layout == "padded" else dict.fromkeys(PAD, 0)
    M, N = data[0]["R1"].shape
    K = data[0]["B"].shape[1]
    c = types.SimpleNamespace(layout=layout, M=M, N=N, K=K, groups=len(data),
                              lda=K + p["lda"], ldb=K + (0 if b_rows_only else p["ldb"]),
                              ldc=N + p["ldc"], ldr1=N + p["ldr1"], ldr2=N + p["ldr2"],
                              ldc2=N + p["ldc2"], pad=p, A=[], B=[], bias=[], R1=[], R1h=[], R2=[],
                              img=[])
    for d in data:
        if d["A"].dim() == 2:
            c.A.append(_pad2(d["A"], c.lda))
        else:          # the image between two NaN guard images of one allocation
            buf = torch.full((d["A"].shape[0] + 2,) + tuple(d["A"].shape[1:]), math.nan,
                             dtype=torch.float16, device=d["A"].device)
            buf[1:-1] = d["A"]
            c.img.append(buf)
            c.A.append(buf[1:])
        c.B.append(_pad2(d["B"], c.ldb))
        bias = torch.full((N + 8,), math.nan, device=d["bias"].device)
        bias[:N] = d["bias"]
        c.bias.append(bias)
        c.R1.append(_pad2(d["R1"], c.ldr1))
        c.R1h.append(_pad2(d["R1"].half(), c.ldr1))
        c.R2.append(_pad2(d["R2"], c.ldr2))
    return c


def make_case(family, M, N, K, groups, layout="padded", **kw):
    b_rows_only = kw.pop("b_rows_only", False)
    return embed(make_data(family, M, N, K, groups, **kw), layout, b_rows_only)


def new_out(shape, dtype, device):
    """An output allocation filled with the sentinel of its type."""
    o = torch.empty(shape, dtype=dtype, device=device)
    fill_sentinel(o)
    return o


def fill_sentinel(o):
    if o.dtype == torch.float16:
        o.view(torch.int16).fill_(SENTINEL16)
    else:
        o.view(torch.int32).fill_(SENTINEL32)


def is_sentinel(o):
    if o.dtype == torch.float16:
        return o.view(torch.int16) == SENTINEL16
    return o.view(torch.int32) == SENTINEL32


def footprint(o, M, N, what="C"):
    """o [M + SPARE, ld] pre-filled with the sentinel: padding columns and
    spare rows untouched, no sentinel left inside M x N.  Returns a list of
    complaints."""
    s = is_sentinel(o)
    bad = []
    if not bool(s[M:].all()):
        bad.append(f"{what}: a store landed in the spare rows")
    if not bool(s[:, N:].all()):
        bad.append(f"{what}: a store landed in the padding columns")
    left = int(s[:M, :N].sum())
    if left:
        bad.append(f"{what}: {left} valid elements were never written")
    return bad


# ------------------------------------------------------------------ shapes ---
def tile0():
    """Tile 0, the static 32x32x16 choice of net_gemm_t1.hip (64x64x64 at these
    sizes), as a table entry."""
    return types.SimpleNamespace(id=0, bm=64, bn=64, bk=64, kg=1, mf=32, regs_epilogue=0, halo=0,
                                 bdirect=0, tail_ok=1, tuner=0)


def dense_axes(t):
    q = 32 if t.bdirect else 8          # B-direct: K % 32 == 0
    Ms = [1, t.bm - 1, t.bm + 1, 2 * t.bm + 3]
    Ns = [8, t.bn - 8, t.bn + 8, 2 * t.bn + 24]
    Ks = [q, t.bk - q, t.bk, t.bk + q, t.kg * t.bk - q, t.kg * t.bk + q, 7 * t.bk + 3 * q]
    return Ms, Ns, list(dict.fromkeys(Ks)), [1, 2, 3]


def dense_shapes(t):
    """(M, N, K, split_k, groups) of a dense tile: two passes over the K list
    with M, N, split and groups cycling at different strides, so that every
    value of every axis appears at least twice and with a tail in every other
    axis; then the all-largest shape with split 3, and one K tile split three
    ways (plan_grid collapses it).  Tile 0 gets the lists of a 64x64x64 and
    of a 128x128x64 tile."""
    Ms, Ns, Ks, Ss = dense_axes(t)
    out = []
    n = len(Ks)
    for i in range(2 * n):
        p = i // n
        out.append((Ms[(i + p) % 4], Ns[(i + 2 * p + 1) % 4], Ks[i % n], Ss[(i + p) % 3], 1 + i % 4))
    out.append((Ms[-1], Ns[-1], Ks[-1], 3, 4))
    out.append((Ms[1], Ns[2], Ks[0], 3, 2))
    out = list(dict.fromkeys(out))
    if t.id == 0 and t.bm == 64:
        big = tile0()
        big.bm = big.bn = 128
        out += [s for s in dense_shapes(big) if s not in out]
    return out


def odd_n_shapes(t):
    """N % 8 != 0: the per-register epilogue (32x32x16 tiles only)."""
    return [(t.bm + 1, t.bn - 3, t.bk + (32 if t.bdirect else 8), 1, 2),
            (2 * t.bm + 3, t.bn + 1, 2 * t.bk, 2, 1)]


def conv_shapes(t):
    """Implicit-conv cases dict(Bn, H, W, C, k, stride, pad, relu_in, Cout): every
    image size, kernel, stride, Cin, relu_in and Cout at least twice."""
    out = []
    hw = [(1, 1), (3, 5), (7, 9)]
    i = 0
    for k in (1, 3):
        for stride in (1, 2):
            for cin in (8, 72, 136):
                H, W = hw[i % 3]
                out.append(dict(Bn=2, H=H, W=W, C=cin, k=k, stride=stride, pad=k // 2,
                                relu_in=bool((i + i // 3) % 2), Cout=8 if i % 2 else t.bn + 8))
                i += 1
        hw = hw[1:] + hw[:1]
    out.append(dict(Bn=2, H=7, W=9, C=136, k=3, stride=1, pad=1, relu_in=True, Cout=t.bn + 8))
    return out


def halo_shapes(t):
    """3x3 / stride 1 / pad 1 cases of a halo tile: W in {bm, 2 bm}, H in
    {1, 2, 3}, Bn in {1, 2}, Cin in {64, 192}, Cout in {8, bn-8, bn, bn+8}."""
    out = []
    couts = [8, t.bn - 8, t.bn, t.bn + 8]
    for i in range(8):
        out.append(dict(Bn=1 + i % 2, H=1 + i % 3, W=t.bm * (1 + (i // 2) % 2), C=(64, 192)[(i // 4 + i) % 2],
                        k=3, stride=1, pad=1, relu_in=bool(i % 2), Cout=couts[i % 4]))
    return out


def expected_refusal(t, *, N, K, conv=None, vec=True, tail=False, tail_n=8, split_k=1, packed_b=True,
                     store="plain"):
    """The s3n_gemm error text a launch must raise, or None when it must run.
    One line per rule of include/s3n.h and of the launchers' S3_REQUIREs.
    vec: the host finds the vector epilogue usable (N % 8 == 0, every ld % 8
    == 0, aligned bases, plain store or ConvT with sCout % 8 == 0, debug 16
    off)."""
    if tail and not (tail_n in (8, 16) and split_k <= 1 and store == "plain"):
        return "tail needs tail_n"                       # net_gemm.hip: tail arguments
    if tail and not vec:
        return "fused tail needs the vector epilogue"    # net_gemm.hip
    if t.halo:
        if not (conv and conv["k"] == 3 and conv["stride"] == 1 and conv["pad"] == 1):
            return "halo tiles need a 3x3"               # launch_halo: 3x3 / stride 1 / pad 1 conv
        if conv["C"] % 64 or conv["W"] % t.bm:
            return "halo tiles need Cin"                 # launch_halo: Cin % 64, BM | width
        if split_k > 1 or not vec or store != "plain":
            return "halo tiles need split_k 1"           # launch_halo: split 1, vector epilogue, plain
        if tail and N != t.bn:
            return "fused tail needs N == BN"            # launch_halo
        return None
    if t.bdirect:
        if conv or not packed_b or not vec or tail or K % 32:
            return "B-direct tiles need"                 # launch_bd: dense A, Bp, vector epilogue, K % 32
        return None
    if t.mf == 16 and not vec:
        return "16x16 MFMA tiles need the vector epilogue"   # launch / launch_pp
    if tail:
        if t.id == 0:
            return None if N in (64, 128) else "fused tail needs N of 64 or 128"   # launch_t1
        if N != t.bn:
            return "fused tail needs N == the tile width"                         # launch / launch_pp
        if t.regs_epilogue:
            return "fused tail needs a tile whose fp32 image fits"                # launch / launch_pp
        if t.kg > 1:
            return "fused tail runs with one K-group"                             # launch
    return None


# --------------------------------------------------------------- emulation ---
def erf_as(x):
    """erf by Abramowitz & Stegun 7.1.26 in fp32, as erf_fast computes it."""
    a = x.abs()
    t = 1.0 / (0.3275911 * a + 1.0)
    q = 1.061405429 * t - 1.453152027
    q = q * t + 1.421413741
    q = q * t - 0.284496736
    q = q * t + 0.254829592
    q = q * t
    e = torch.exp2(-(a * a) * 1.4426950408889634)
    return torch.copysign(1.0 - q * e, x)


def emulate(A, B, bias=None, act="none", R1=None, f16_out=False, chunk=32, bk=64, kg=1, split=1,
            defect=None):
    """The kernels' arithmetic in fp32 on the CPU: products of `chunk` k (one
    MFMA) accumulated in K order inside a K tile, K-group g taking the K tiles
    g, g + kg, ..., groups then splits summed in order, the epilogue in fp32
    with the A&S erf.  A [M,K], B [N,K] fp16.  defect plants an error:
    'acc_f16' (accumulator rounded to fp16 before the bias), 'tanh' (tanh GELU),
    'drop_k' (one k term lost), 'bias_next' (bias of column j+1), 'relu_late'
    (act applied after the residual)."""
    a, b = A.float(), B.float()
    M, K = a.shape
    if defect == "drop_k":
        a = a.clone()
        a[:, K // 2] = 0
    kt = -(-K // bk)
    per = -(-kt // max(1, split))
    total = None
    for s in range(-(-kt // per)):
        tiles = range(s * per, min(kt, (s + 1) * per))
        part = None
        for g in range(kg):
            acc = torch.zeros(M, b.shape[0])
            for t in list(tiles)[g::kg]:
                for k0 in range(t * bk, min(K, (t + 1) * bk), chunk):
                    acc = acc + a[:, k0:k0 + chunk] @ b[:, k0:k0 + chunk].T
            part = acc if part is None else part + acc
        total = part if total is None else total + part
    v = total
    if defect == "acc_f16":
        v = v.half().float()
    if bias is not None:
        v = v + (torch.roll(bias, -1) if defect == "bias_next" else bias)
    late = defect == "relu_late" and R1 is not None
    if late:
        v = v + R1.float()
    if act == "gelu":
        if defect == "tanh":
            v = 0.5 * v * (1 + torch.tanh(0.7978845608 * (v + 0.044715 * v ** 3)))
        else:
            v = 0.5 * v * (1.0 + erf_as(v * 0.70710678118654752))
    elif act == "relu":
        v = v.clamp_min(0)
    if R1 is not None and not late:
        v = v + R1.float()
    return v.half() if f16_out else v
