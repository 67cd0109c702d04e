"""Float64 references, derived per-element bounds, input families, fp32 CPU
emulations and deliberately wrong variants for the memory-bound network
kernels of csrc/net_ops.hip (include/s3n.h): LayerNorm, bilinear x2 upsample,
Gaussian-head postprocess, fp32 -> fp16 cast, patch im2col and the PRNG fill.
For tests/test_net_ops_edges.py.

Plain PyTorch / numpy on the CPU.  Every reference is the operation's
definition in float64 from the exact input bits; nothing of the kernels' lane
layout is restated in a reference.  The bounds below come from the fp32
evaluation order (net_ops.hip is built without fma contraction, so every
operator rounds once), with u = 2^-24 the unit roundoff of fp32.  None of
them is fitted to measured results and none carries a safety factor.

Transcendentals: the "AMD Instinct CDNA3/CDNA4 Instruction Set Architecture"
reference gives V_RSQ_F32, V_EXP_F32, V_RCP_F32 and V_SQRT_F32 1 ULP of
accuracy, and the HIP programming guide's math-API accuracy table gives
rsqrtf, expf, expm1f and sqrtf a maximum error of 1 ULP.  One ULP is at most
2u relative.  fp32 division and sqrtf are compiled correctly rounded (hipcc's
default), u relative; the bounds grant them the 1 ULP = 2u of the table only
where noted.

LayerNorm  y = (x - mu) rsqrt(var + eps) gamma + beta, one row of C values.
  L = log2(C) + 2 is the depth of the lane sum plus the butterfly.
  * mean:      dmu   = L u mean|x|
  * d = x-mu:  dd_i  = 2u |d_i| + dmu
  * variance:  dvar  = (L + 3) u var + mean_i(2 |d_i| dd_i)
               (the three extra roundings: the square, the division by C and
               the addition of eps)
  * rstd:      rel_r = dvar / (2 (var + eps)) + 2u      (rsqrtf: 1 ULP = 2u)
  * product p = d r gamma, three roundings, and one on the add of beta:
      b32_i = |gamma_i| r dd_i + |p_i| rel_r + 3u |p_i| + u |y_i|
  * fp16 output: b16_i = b32_i + 2^-11 (|y_i| + b32_i) + 2^-25
    (2^-25: half the smallest fp16 subnormal).
  eps is the fp32 value the kernel receives.  On the N(0,1) family the fp32
  bound is about 2e-6 of max|y|.
  L is the depth of a balanced reduction.  The kernel's per-lane part is a
  chain (V + 2 adds for the sum, 4V for the squares, V = ceil(C / 256)), which
  for C > 1024 is deeper than L; a strict worst case would put 6 + 4V in the
  place of L + 3.  The bound keeps L: the terms of a chain of positive squares
  would all have to round the same way to get there, and tightening matters
  more here than covering that corner (the oracle's one-pass variant sits
  only 4x to 15x outside on the 3e4 family).

Upsample (align_corners=True, scale from 2H and 2W, top-left crop).  The
source coordinate of output row oy is the exact rational oy (H-1) / (2H-1):
floor and fraction are taken in integer arithmetic.
  * weights: fy = sh * oy carries the rounding of sh and of the product, and
    1 - ly one more: dw_y = 3u max(fy, 1), likewise dw_x.  A weight error
    moves the result by at most dw times the spread S (max - min) of the
    inputs around the source point.  At an integer coordinate the fp32 floor
    may land one cell before the exact one (the result is continuous there,
    the taps are not), so S is taken over rows y0-1 .. y0+2 and columns
    x0-1 .. x0+2, clamped to the image.
  * blend: every tap passes a product, an add, a product and an add:
    4u A with A = sum |tap| weight.
  * t32 = (dw_y + dw_x) S + 4u A;  tol = t32 + 2^-11 (|ref| + t32) + 2^-25.

Postprocess, relative per element unless noted, plus an absolute floor of
2^-126 (the smallest normal fp32: a flushed denormal is not an error).
  n(v) = |v|: k squares (u each) and k - 1 sequential adds give the sum
  (1 + (k-1)) u, halved by the root, plus the root's 2u:
  xyz / offsets (k = 3): 3.5u, quaternion (k = 4): 4u, descriptor (k = 24): 14u.
  * pts3d = xyz / max(d, 1e-8f) expm1(d): the clip keeps d's 3.5u; expm1
    amplifies it by kappa(d) = d e^d / (e^d - 1) (between 1 and d + 1) and
    adds its own 2u; the division and the product one u each:
    (7.5 + 3.5 kappa) u, taken as (8 + 4 kappa) u.
  * conf, desc_conf = 1 + exp(l): 2u on exp, u on the add: 3u.
  * scales = exp(l): 2u.
  * opacities = 1 / (1 + exp(-l)): 2u + u + u = 4u.
  * rotations = q / (|q| + 1e-8f): 4u + u + u = 6u.
  * desc = f (1 / |f|): 14u + u + u = 16u.  A zero row is NaN in all 24.
  * sh: a copy, bit-exact.
  * means = pts3d + dir (exp(od - 6) - exp(-6)), dir = off / max(od, 1e-8f).
    The difference cancels for small od (in the original fp32 formulation as
    much as here), so its term is absolute: with E1 = exp(od - 6),
    E0 = exp(-6), od - 6 is off by 3.5u od + u |od - 6|, hence
      dof = u (E1 (2 + 3.5 od + |od - 6|) + 2 E0 + |of|)
    and the offset's error is |dir| dof + 5.5u |dir of| (dir: 3.5u + u, the
    product u); the final add rounds once more: u |means|.
    use_offsets = 0: means is pts3d.
  The float clips are the fp32 constant 1e-8f in the reference too.

Cast, im2col and PRNG are bit-exact: x.half(); the [B, Ht, Wt, c, ky, kx]
regrouping of the image rounded to fp16 (F.unfold's order); the header's
formula restated with Python integers masked to 64 bits and numpy fp32 steps.

Worst err / bound of the CPU emulations below over every family and shape
of the GPU tests (test_oracle_emulations_stay_inside_the_bounds):
layernorm fp32 / fp16 output: normal 0.90 / 0.995, offset1000 0.49 / 0.94,
offset3e4 0.19 / 0.28, constant 0.43 / 0.97, spike 0.96 / 0.997, tiny 0.97 /
0.998; upsample: random 0.992, index 0.993, pm60000 0.887, subnormal 0.996;
postprocess: pts3d 0.35, conf 0.50, desc 0.28, desc_conf 0.50, scales 0.50,
rotations 0.42, opacities 0.48, means 0.53, sh 0 (exact).  Where one
rounding dominates a bound (the fp16 store; the final add of beta when
|beta| >> |p|), a figure close to 1 is the half-ulp worst case of that
rounding and not slack used up elsewhere.

Measured on the MI355X, worst err / bound per kernel and family over all
cases of tests/test_net_ops_edges.py:
layernorm fp32 / fp16 output: normal 0.90 / 0.99, offset1000 0.18 / 0.94,
offset3e4 0.14 / 0.28, constant 0.21 / 0.97, spike 0.95 / 1.00, tiny 0.97 /
1.00 (0.997 and 0.998 before rounding to two digits); upsample: random 0.992,
index 0.993, pm60000 0.887, subnormal 0.996, the same as the emulation, and
the 1- and 4-pixel-per-thread kernels equal the 2-pixel one bit for bit; postprocess per output over all
families: pts3d 0.35, conf 0.52, desc 0.28, desc_conf 0.55, scales 0.66,
rotations 0.42, opacities 0.52, means 0.55, sh 0; per family over all
outputs: normal 0.64, small 0.65, large 0.65, logits 0.41, quat 0.62,
descnorm 0.66.  Cast, im2col and PRNG: bit-exact on every case.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
H_EPS = 2.0 ** -11
H_SUB = 2.0 ** -25
FLT_MIN = 2.0 ** -126
CLIP = float(np.float32(1e-8))

# bit patterns of NaNs no kernel produces (hardware NaNs are 0x7FC00000 /
# 0x7E00 up to sign): unwritten output is recognisable bit for bit
SENT32 = 0x7FC5A5A5
SENT16 = 0x7E5A

f32 = np.float32


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 12345) % (2 ** 62)
    return torch.Generator().manual_seed(s)


def worst_ratio(got, ref, tol):
    """Worst |got - ref| / tol.  NaN where the reference is NaN counts as
    agreement, NaN anywhere else (or a missing NaN) as an infinite ratio; a
    zero bound demands equality."""
    got, ref, tol = (torch.as_tensor(t).double().reshape(-1) for t in (got, ref, tol))
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    ratio = torch.where(tol > 0, err / tol, torch.where(err == 0, 0.0, math.inf))
    rn, gn = ref.isnan(), got.isnan()
    ratio = torch.where(rn & gn, torch.zeros_like(ratio), ratio)
    ratio = torch.where(rn ^ gn, torch.full_like(ratio, math.inf), ratio)
    ratio = torch.where(ratio.isnan(), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max())


# ================================================================ LayerNorm ===
LN_FAMILIES = ("normal", "offset1000", "offset3e4", "constant", "spike", "tiny")
LN_EPS = 1e-6


def ln_inputs(family, rows, C, groups, seed=0):
    """Per group (x [rows, C], gamma [C], beta [C]) fp32; every group has its
    own data and its own gamma / beta."""
    assert family in LN_FAMILIES, family
    out = []
    for g in range(groups):
        gen = _gen(seed, g, LN_FAMILIES.index(family), rows, C)
        rn = lambda *s: torch.randn(*s, generator=gen)
        x = rn(rows, C)
        if family == "offset1000":
            x = 1000 + x
        elif family == "offset3e4":
            x = 3e4 + 0.01 * x
        elif family == "constant":
            x = (3 * rn(rows, 1)).expand(rows, C).clone()
        elif family == "spike":
            if rows:
                x[torch.arange(rows), torch.randint(0, C, (rows,), generator=gen)] = 1e4
        elif family == "tiny":
            x = 1e-4 * x
        out.append((x.float().contiguous(), 1 + 0.5 * rn(C), rn(C)))
    return out


def ln_reference(x, gamma, beta, eps=LN_EPS):
    """(y, b32, b16) float64 [rows, C]: the definition and the two bounds of
    the module docstring."""
    eps = float(f32(eps))
    C = x.shape[-1]
    L = math.log2(C) + 2
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    r = (var + eps).rsqrt()
    p = d * r * g
    y = p + b
    dmu = L * U * x.abs().mean(-1, keepdim=True)
    dd = 2 * U * d.abs() + dmu
    dvar = (L + 3) * U * var + (2 * d.abs() * dd).mean(-1, keepdim=True)
    rel_r = dvar / (2 * (var + eps)) + 2 * U
    b32 = g.abs() * r * dd + p.abs() * rel_r + 3 * U * p.abs() + U * y.abs()
    b16 = b32 + H_EPS * (y.abs() + b32) + H_SUB
    return y, b32, b16


def ln_padded_width(C):
    """Columns a wave's registers cover: 256 per float4 vector of a lane, with
    1, 2, 3, 4 or 8 vectors."""
    v = -(-C // 256)
    return 256 * (v if v <= 4 else 8)


LN_WRONG = ("one_pass", "padded_width", "no_eps", "group0_affine")


def ln_emulate(inputs, eps=LN_EPS, wrong=None):
    """Two-pass LayerNorm in fp32, operator by operator, for every group of
    `inputs`; returns per group (y32 fp32, y16 fp16).  `wrong` selects one of
    LN_WRONG."""
    assert wrong is None or wrong in LN_WRONG
    out = []
    eps = f32(0.0) if wrong == "no_eps" else f32(eps)
    for gi, (x, gamma, beta) in enumerate(inputs):
        if wrong == "group0_affine":
            gamma, beta = inputs[0][1], inputs[0][2]
        x, g, b = x.numpy(), gamma.numpy(), beta.numpy()
        C = x.shape[-1]
        div = f32(ln_padded_width(C) if wrong == "padded_width" else C)
        with np.errstate(all="ignore"):
            mean = (x.sum(-1, keepdims=True, dtype=f32) / div).astype(f32)
            d = (x - mean).astype(f32)
            if wrong == "one_pass":
                var = ((x * x).astype(f32).sum(-1, keepdims=True, dtype=f32) / div
                       - mean * mean).astype(f32)
            else:
                var = ((d * d).astype(f32).sum(-1, keepdims=True, dtype=f32) / div).astype(f32)
            rstd = (f32(1.0) / np.sqrt((var + eps).astype(f32))).astype(f32)
            y = (((d * rstd).astype(f32) * g).astype(f32) + b).astype(f32)
        y = torch.from_numpy(y)
        out.append((y, y.clamp(-65504.0, 65504.0).half()))
    return out


# ================================================================= upsample ===
UP_SHAPES = ((1, 1, 1, 1), (1, 1, 2, 2), (1, 5, 2, 9), (5, 1, 9, 2), (2, 3, 4, 6), (2, 3, 3, 5),
             (5, 7, 9, 13), (5, 7, 10, 14), (12, 16, 24, 31))
UP_FAMILIES = ("random", "index", "pm60000", "subnormal")


def up_cases():
    """(family, H, W, oh, ow, C, B, groups): every shape with every family;
    C, B and groups cycle so that every value meets every shape class."""
    Cs, Bs, Gs = (8, 16, 128), (1, 3), (1, 2, 4)
    out = []
    for i, (H, W, oh, ow) in enumerate(UP_SHAPES):
        for j, fam in enumerate(UP_FAMILIES):
            out.append((fam, H, W, oh, ow, Cs[(i + j) % 3], Bs[(i + j // 2 + i // 3) % 2],
                        Gs[(i // 3 + 2 * j + i) % 3]))
    return out


def up_guard(W, C):
    """Elements of NaN guard behind every input: one row and one pixel, what
    an unclamped x1 / y1 would reach."""
    return (W + 1) * C


def up_inputs(family, B, H, W, C, groups, seed=0):
    """Per group a flat fp16 buffer: the [B, H, W, C] image followed by
    up_guard(W, C) NaNs that no result may depend on."""
    assert family in UP_FAMILIES, family
    out = []
    n = B * H * W * C
    for g in range(groups):
        gen = _gen(seed, g, UP_FAMILIES.index(family), B, H, W, C)
        if family == "random":
            x = torch.randn(n, generator=gen).half()
        elif family == "index":
            # the fp16 bit pattern 0x3C00 + 37 code mod 8192 (1.0 .. 255.9) is a
            # distinct value for every code (b, y, x, c mod 8) < 8192
            b, y, xx, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W),
                                         torch.arange(C), indexing="ij")
            code = ((b * H + y) * W + xx) * 8 + c % 8
            assert int(code.max()) < 8192
            bits = 0x3C00 + (code * 37 + 1000 * g) % 8192
            x = bits.to(torch.int16).view(torch.float16).reshape(-1)
            if g % 2:
                x = -x
        elif family == "pm60000":
            b, y, xx, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W),
                                         torch.arange(C), indexing="ij")
            x = (60000.0 * (1 - 2 * ((b + y + xx + c + g) % 2))).half().reshape(-1)
        else:
            bits = torch.randint(1, 0x400, (n,), generator=gen)
            bits = bits + 0x8000 * torch.randint(0, 2, (n,), generator=gen)
            x = bits.to(torch.int32).to(torch.int16).view(torch.float16)
        guard = torch.full((up_guard(W, C),), math.nan, dtype=torch.float16)
        out.append(torch.cat([x, guard]))
    return out


def _up_axis(n_in, n_out):
    """Exact taps of one axis: (i0, i1, frac, coordinate) for outputs 0..n_out-1."""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = o * (n_in - 1), 2 * n_in - 1
    i0 = num // den
    frac = (num % den).double() / den
    return i0, (i0 + 1).clamp(max=n_in - 1), frac, num.double() / den


def up_reference(x, B, H, W, C, oh, ow):
    """x: flat fp16 (guard allowed).  (ref, tol) float64 [B, oh, ow, C]."""
    img = x[:B * H * W * C].reshape(B, H, W, C).double()
    y0, y1, ly, fy = _up_axis(H, oh)
    x0, x1, lx, fx = _up_axis(W, ow)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    hy, hx = 1 - ly, 1 - lx

    def blend(im):
        a, b = im[:, y0][:, :, x0], im[:, y0][:, :, x1]
        c, d = im[:, y1][:, :, x0], im[:, y1][:, :, x1]
        return hy * (hx * a + lx * b) + ly * (hx * c + lx * d)

    ref, A = blend(img), blend(img.abs())
    hi = torch.full_like(ref, -math.inf)
    lo = torch.full_like(ref, math.inf)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            t = img[:, (y0 + dy).clamp(0, H - 1)][:, :, (x0 + dx).clamp(0, W - 1)]
            hi, lo = torch.maximum(hi, t), torch.minimum(lo, t)
    dw = (3 * U * fy.clamp(min=1))[None, :, None, None] + (3 * U * fx.clamp(min=1))[None, None, :, None]
    t32 = dw * (hi - lo) + 4 * U * A
    return ref, t32 + H_EPS * (ref.abs() + t32) + H_SUB


UP_WRONG = ("align_corners_false", "scale_from_crop", "no_clamp", "skip_tail")


def up_emulate(x, B, H, W, C, oh, ow, wrong=None):
    """The kernel's per-pixel arithmetic in fp32 (coordinates in fp32, (int)
    truncation) on the flat buffer `x`, which must carry the NaN guard: an
    unclamped tap reads whatever follows in memory.  fp16 [B, oh, ow, C];
    pixels a wrong variant leaves unwritten are NaN."""
    assert wrong is None or wrong in UP_WRONG
    xf = x.float()

    def axis(n_in, n_crop):
        o = torch.arange(n_crop, dtype=torch.float32)
        if wrong == "align_corners_false":
            f = ((o + 0.5) * 0.5 - 0.5).clamp(min=0)
        else:
            n_out = n_crop if wrong == "scale_from_crop" else 2 * n_in
            s = (torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1))
                 if n_out > 1 else torch.tensor(0.0))
            f = s * o
        i0 = f.to(torch.int64)
        i1 = i0 + 1 if wrong == "no_clamp" else (i0 + 1).clamp(max=n_in - 1)
        l = f - i0.float()
        return i0, i1, l, 1.0 - l

    y0, y1, ly, hy = axis(H, oh)
    x0, x1, lx, hx = axis(W, ow)
    b = torch.arange(B)[:, None, None, None]
    c = torch.arange(C)[None, None, None, :]

    def tap(yy, xx):
        idx = ((b * H + yy[None, :, None, None]) * W + xx[None, None, :, None]) * C + c
        return xf[idx]

    ly, hy = ly[None, :, None, None], hy[None, :, None, None]
    lx, hx = lx[None, None, :, None], hx[None, None, :, None]
    o = hy * (hx * tap(y0, x0) + lx * tap(y0, x1)) + ly * (hx * tap(y1, x0) + lx * tap(y1, x1))
    o = o.half()
    if wrong == "skip_tail" and ow % 2:
        o[:, :, ow - 1] = math.nan
    return o


# ============================================================== postprocess ===
PP_FAMILIES = ("normal", "small", "large", "logits", "quat", "descnorm")
PP_OUT = dict(pts3d=3, conf=1, desc=24, desc_conf=1, scales=3, rotations=4, sh=3, opacities=1,
              means=3)


def _unit_rows(gen, n, k):
    v = torch.randn(n, k, generator=gen, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True).clamp(min=1e-300)


def pp_inputs(family, n, ld_pts, ld_g, seed=0):
    """(pts [n, ld_pts], feat [n, 25], gauss [n, ld_g]) fp32.  Columns past
    the 4 / 14 the kernel may read are NaN."""
    assert family in PP_FAMILIES, family
    gen = _gen(seed, PP_FAMILIES.index(family), n, ld_pts, ld_g)
    pts = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    feat = torch.randn(n, 25, generator=gen, dtype=torch.float64)
    gs = torch.randn(n, 14, generator=gen, dtype=torch.float64)
    i = torch.arange(n)
    if family == "small":
        for dst in (pts, gs):
            mag = 10.0 ** (-12 + 10 * torch.rand(n, 1, generator=gen, dtype=torch.float64))
            dst[:, :3] = _unit_rows(gen, n, 3) * mag
        pts[i % 7 == 3, :3] = 0.0
        gs[i % 7 == 5, :3] = 0.0
        if n:
            pts[n - 1, :3] = 0.0
            gs[n - 1, :3] = 0.0
    elif family == "large":
        pts[:, :3] = _unit_rows(gen, n, 3) * (1 + 59 * torch.rand(n, 1, generator=gen, dtype=torch.float64))
        pts[:, :3] *= 1 - 2.0 ** -20          # fp32 rounding cannot push the norm above 60
    elif family == "logits":
        lv = torch.tensor([20.0, -20.0, 80.0, -80.0], dtype=torch.float64)
        pts[:, 3] = lv[i % 4]
        feat[:, 24] = lv[(i + 1) % 4]
        for k in range(3):
            gs[:, 3 + k] = lv[(i + 2 + k) % 4]
        ov = torch.tensor([20.0, -20.0, 80.0, -80.0, 100.0, -100.0], dtype=torch.float64)
        gs[:, 13] = ov[(i + n) % 6]
    elif family == "quat":
        qn = torch.tensor([1e-9, 1e-4, 1.0], dtype=torch.float64)
        gs[:, 6:10] = _unit_rows(gen, n, 4) * qn[(i + n) % 3][:, None]
    elif family == "descnorm":
        dn = torch.tensor([1e-15, 1e15], dtype=torch.float64)
        feat[:, :24] = _unit_rows(gen, n, 24) * dn[i % 2][:, None]
        if n:
            feat[n // 2, :24] = 0.0
    P = torch.full((n, ld_pts), math.nan)
    G = torch.full((n, ld_g), math.nan)
    P[:, :4], G[:, :14] = pts.float(), gs.float()
    return P, feat.float().contiguous(), G


def pp_reference(pts, feat, gauss, use_offsets):
    """name -> (ref, tol) float64, shaped like the kernel's outputs."""
    P, Fe, G = pts[:, :4].double(), feat.double(), gauss[:, :14].double()
    xyz = P[:, :3]
    d = xyz.norm(dim=-1, keepdim=True)
    kappa = torch.where(d > 0, d * d.exp() / torch.expm1(d).clamp(min=1e-300), torch.ones_like(d))
    kappa = torch.where(d > 1e-6, kappa, torch.ones_like(d))
    p3 = xyz / d.clamp(min=CLIP) * torch.expm1(d)
    t3 = (8 + 4 * kappa) * U * p3.abs()
    off = G[:, :3]
    od = off.norm(dim=-1, keepdim=True)
    dirn = off / od.clamp(min=CLIP)
    E1, E0 = (od - 6).exp(), math.exp(-6.0)
    of = E0 * torch.expm1(od)
    dof = U * (E1 * (2 + 3.5 * od + (od - 6).abs()) + 2 * E0 + of.abs())
    offs = dirn * of
    toff = dirn.abs() * dof + 5.5 * U * offs.abs()
    q = G[:, 6:10]
    fn = Fe[:, :24].norm(dim=-1, keepdim=True)
    desc = torch.where(fn > 0, Fe[:, :24] / fn, torch.full_like(Fe[:, :24], math.nan))
    ref = dict(pts3d=p3, conf=1 + P[:, 3].exp(), desc=desc, desc_conf=1 + Fe[:, 24].exp(),
               scales=G[:, 3:6].exp(), rotations=q / (q.norm(dim=-1, keepdim=True) + CLIP),
               sh=G[:, 10:13], opacities=torch.sigmoid(G[:, 13]))
    rel = dict(conf=3, desc=16, desc_conf=3, scales=2, rotations=6, opacities=4)
    out = {k: (v, rel[k] * U * v.abs() + FLT_MIN) for k, v in ref.items() if k in rel}
    out["pts3d"] = (p3, t3 + FLT_MIN)
    out["sh"] = (ref["sh"], torch.zeros_like(ref["sh"]))
    if use_offsets:
        m = p3 + offs
        out["means"] = (m, t3 + toff + U * m.abs() + FLT_MIN)
    else:
        out["means"] = (p3, t3 + FLT_MIN)
    return out


PP_WRONG = ("exp_minus_1", "no_clip", "no_quat_eps", "offsets_ignored")


def pp_emulate(pts, feat, gauss, use_offsets, wrong=None):
    """The kernel's formulas in fp32, operator by operator; exp and expm1 are
    taken in float64 and rounded (numpy's own float32 exp is a 2.5 ULP
    routine, less than the 1 ULP the bound grants); name -> fp32 tensor."""
    assert wrong is None or wrong in PP_WRONG
    P, Fe, G = pts.numpy()[:, :4], feat.numpy(), gauss.numpy()[:, :14]
    one, clip = f32(1.0), f32(1e-8)
    exp = lambda v: np.exp(np.asarray(v, dtype=np.float64)).astype(f32)
    expm1 = lambda v: np.expm1(np.asarray(v, dtype=np.float64)).astype(f32)
    if wrong == "offsets_ignored":
        use_offsets = not use_offsets

    def norm(v):
        s = (v[:, 0] * v[:, 0]).astype(f32)
        for k in range(1, v.shape[1]):
            s = (s + (v[:, k] * v[:, k]).astype(f32)).astype(f32)
        return np.sqrt(s).astype(f32)[:, None]

    with np.errstate(all="ignore"):
        xyz = P[:, :3]
        d = norm(xyz)
        dc = d if wrong == "no_clip" else np.maximum(d, clip)
        e = (exp(d) - one).astype(f32) if wrong == "exp_minus_1" else expm1(d)
        p3 = ((xyz / dc).astype(f32) * e).astype(f32)
        off = G[:, :3]
        od = norm(off)
        odc = od if wrong == "no_clip" else np.maximum(od, clip)
        of = (exp((od - f32(6.0)).astype(f32)) - exp(f32(-6.0))).astype(f32)
        q = G[:, 6:10]
        qn = norm(q) if wrong == "no_quat_eps" else (norm(q) + clip).astype(f32)
        inv = (one / norm(Fe[:, :24])).astype(f32)
        out = dict(pts3d=p3, conf=(one + exp(P[:, 3])).astype(f32),
                   desc=(Fe[:, :24] * inv).astype(f32),
                   desc_conf=(one + exp(Fe[:, 24])).astype(f32),
                   scales=exp(G[:, 3:6]), rotations=(q / qn).astype(f32),
                   sh=G[:, 10:13].copy(),
                   opacities=(one / (one + exp(-G[:, 13])).astype(f32)).astype(f32))
        out["means"] = (p3 + ((off / odc).astype(f32) * of).astype(f32)).astype(f32) if use_offsets else p3
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


# ===================================================================== cast ===
CAST_FAMILIES = ("f16_images", "midpoints", "subnormal", "edges")
CAST_SHAPES = ((1, 1, 1, 1), (3, 5, 5, 5), (7, 37, 40, 64), (5, 256, 256, 300), (2, 257, 260, 257))


def cast_values(family):
    """1-D fp32 tensor of the family's values."""
    assert family in CAST_FAMILIES, family
    if family == "f16_images":
        # every fp16 bit pattern (NaNs and infinities included) as fp32
        return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16).float()
    if family == "midpoints":
        # consecutive finite fp16 a < b (subnormals included): (a + b) / 2 is
        # exact in fp32; the midpoint (a tie) and its two fp32 neighbours
        h = torch.arange(0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16).float()
        mid = ((h[:-1].double() + h[1:].double()) / 2).float()
        assert bool((mid.double() * 2 == h[:-1].double() + h[1:].double()).all())
        m = mid.numpy()
        lo, hi = np.nextafter(m, f32(-np.inf)), np.nextafter(m, f32(np.inf))
        v = torch.from_numpy(np.stack([lo, m, hi], 1).reshape(-1))
        return torch.cat([v, -v])
    if family == "subnormal":
        gen = _gen(77)
        k = torch.arange(0, 1025, dtype=torch.float64)
        grid = torch.cat([k, k + 0.5, k + 0.25, k + 0.75]) * 2.0 ** -24
        rnd = 2.0 ** (-30 + 16 * torch.rand(4096, generator=gen, dtype=torch.float64))
        v = torch.cat([grid, rnd, torch.tensor([2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23),
                                                2.0 ** -25 * (1 - 2.0 ** -24), 2.0 ** -26, 1e-45])]).float()
        return torch.cat([v, -v])
    e = np.array([65504.0, -65504.0, np.nextafter(f32(65520.0), f32(0.0)), 65520.0,
                  np.nextafter(f32(65520.0), f32(np.inf)), -65520.0, 65536.0, 1e30, -1e30, np.inf,
                  -np.inf, np.nan, 0.0, -0.0, 65519.0, np.nextafter(f32(65504.0), f32(np.inf))],
                 dtype=f32)
    return torch.from_numpy(e)


def cast_truncate(x):
    """Wrong variant: fp32 -> fp16 rounding toward zero."""
    h = x.half()
    b = h.view(torch.int16).clone()
    over = (h.float().abs() > x.abs()) & ~x.isnan()
    b[over] -= 1          # one step toward zero in sign-magnitude order (inf -> 65504)
    return b.view(torch.float16)


def f16_equal(a, b):
    """Bit equality of fp16 tensors where neither is NaN, and NaN at the same
    places."""
    an, bn = a.isnan(), b.isnan()
    same = a.contiguous().view(torch.int16) == b.contiguous().view(torch.int16)
    return bool((an == bn).all()) and bool((same | an).all())


# =================================================================== im2col ===
IM2COL_SHAPES = ((1, 16, 16, 16), (2, 32, 48, 16), (1, 3, 5, 1), (3, 8, 12, 4), (1, 9, 6, 3))


def im2col_inputs(B, H, W, p, family="index"):
    """[B, 3, H, W] fp32.  index: integers in [-2048, 2048] (exact in fp16),
    idx * 1021 mod 4097 - 2048: distinct while the image has at most 4097
    elements; beyond that the code repeats with period 4097, which no stride
    of the layouts divides.  random: N(0,1), so the store rounds."""
    n = B * 3 * H * W
    if family == "index":
        v = (torch.arange(n, dtype=torch.int64) * 1021) % 4097 - 2048
        return v.float().reshape(B, 3, H, W)
    return torch.randn(n, generator=_gen(B, H, W, p)).reshape(B, 3, H, W)


IM2COL_WRONG = ("kykx_swapped", "channel_last")


def im2col_reference(img, p, wrong=None):
    """A [B Ht Wt, 3 p p] fp16 with k = c p p + ky p + kx."""
    assert wrong is None or wrong in IM2COL_WRONG
    B, _, H, W = img.shape
    t = img.reshape(B, 3, H // p, p, W // p, p)          # b c ty ky tx kx
    order = {None: (0, 2, 4, 1, 3, 5), "kykx_swapped": (0, 2, 4, 1, 5, 3),
             "channel_last": (0, 2, 4, 3, 5, 1)}[wrong]
    return t.permute(*order).reshape(B * (H // p) * (W // p), 3 * p * p).half()


# ===================================================================== PRNG ===
M64 = (1 << 64) - 1
PRNG_NS = (1, 255, 256, 257)
PRNG_AC = ((0.0541, 0.0), (0.0, 0.25), (1.0, -1.0))


def prng_reference(seed, n, a, c):
    """w[i] = (2u - 1) a + c, u = (splitmix64(seed + (i+1) 0x9E3779B97F4A7C15)
    >> 40) 2^-24 (include/s3n.h): 64-bit steps as masked Python integers, the
    float steps one fp32 operator at a time."""
    out = np.empty(n, dtype=f32)
    a, c = f32(a), f32(c)
    for i in range(n):
        z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        u = f32(z >> 40) * f32(2.0 ** -24)
        out[i] = f32(f32(f32(u * f32(2.0)) - f32(1.0)) * a) + c
    return out
