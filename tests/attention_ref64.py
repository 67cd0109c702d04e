"""Float64 reference, derived tolerance and input families for the fused
attention kernels (csrc/net_attn.hip, include/s3n.h), for
tests/test_attention.py.

Plain PyTorch, device agnostic (the oracle tests run it on the CPU, the GPU
tests on the device so the reference is computed once per case and shared by
all kernels).  Nothing of the kernels' tiling is restated in `reference`: it
is softmax(Q K^T scale) V in float64 from the fp16 input bits.

Layout: Q is [B * Nq, H * 64] fp16 rows (batch-major), K and V are
[B * Nk + SPARE, H * 64]: every family carries SPARE = 64 rows behind the last
batch's keys, which no kernel may read into a result.

Tolerance for the kernels without RoPE, per output element (i, d), from the
arithmetic and not from measured results:

    tol = 2^-10 A[i,d] + 2^-11 |ref[i,d]| + Nk 2^-24 max|V|

with A = softmax(...) @ |V|, the scale that one rounding of P acts on.
  * 2^-10 A: P is rounded to fp16 (2^-11 relative) before P V; doubled
    because the row sum is taken over the unrounded P.
  * 2^-11 |ref|: the fp16 rounding of the stored output.
  * Nk 2^-24 max|V|: P below 2^-14 is fp16-subnormal (absolute error up to
    2^-25 per key) or flushed; max|V| is taken per (group, batch, head) over
    the Nk valid keys.
  * The fp32 score / accumulation error and the 1-ulp hardware exponent are
    two orders of magnitude below these as long as
    |score * scale * log2 e| <= 400, which every family respects
    (`max_log2_score` returns the figure; the oracle test asserts it).

The RoPE kernel rotates Q and K in fp32 (the compiler may contract to fma)
and rounds to fp16, so a rotated element may differ by one fp16 ulp from the
reference's (rotated in float64 from the fp32 tables, rounded once).  Worst
case, as if every element were flipped: the score moves by at most
eps_i = scale 2^-10 max_j sum_d |q^_id| |k^_jd|, which moves P and its
normalisation by eps_i each: one more term 2 eps_i A[i,d].

Measured on the MI355X, worst err / tol over all shapes and both layouts of
tests/test_attention.py, as "Nk <= 128 / Nk > 128" (the worst elements sit at
one or two key tiles, where the six kernels without RoPE do the same
arithmetic; above that they differ in the third digit): random 0.37 / 0.25,
random_q4 0.52 / 0.47, onehot8 0.03 / 0.16, onehot32 0.00 / 0.00, ramp_up
0.47 / 0.35, ramp_down 0.45 / 0.35, allneg 0.35 / 0.20, intruder 0.51 / 0.51,
nan 0.39 / 0.26; uniform 0.24 / 0.13 of the bound and at most one fp16 ulp.
RoPE kernel, self / cross positions: at most 0.05 (its worst-case term
dominates the bound).  The CPU emulation `emulate` below reaches 0.38 on the
oracle test's shapes.
"""
import math

import torch

D = 64
KT = 64            # keys per tile in every kernel
SPARE = 64         # rows behind the last batch's keys in every K / V allocation
SCALE = D ** -0.5
LOG2E = 1.4426950408889634

FAMILIES = ("random", "random_q4", "onehot8", "onehot32", "ramp_up", "ramp_down", "uniform",
            "allneg", "intruder", "nan")


# ------------------------------------------------------------------ layout ---
def to_heads(x, B, N, H):
    """[>= B*N, H*64] rows -> [B, H, N, 64] float64 (spare rows dropped)."""
    return x[:B * N].reshape(B, N, H, D).permute(0, 2, 1, 3).double()


def to_rows(x):
    """[B, H, N, 64] -> [B*N, H*64]."""
    B, H, N, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * D)


# --------------------------------------------------------------- reference ---
def reference(qh, kh, vh, scale=SCALE):
    """qh [B,H,Nq,64], kh / vh [B,H,Nk,64] float64 -> (ref, A) [B,H,Nq,64]."""
    P = ((qh @ kh.transpose(-1, -2)) * scale).softmax(-1)
    return P @ vh, P @ vh.abs()


def tolerance(ref, A, vh, eps=None):
    """The bound of the module docstring; eps [B,H,Nq] adds the RoPE term."""
    Nk = vh.shape[2]
    vmax = vh.abs().amax(dim=(2, 3), keepdim=True)
    tol = 2.0 ** -10 * A + 2.0 ** -11 * ref.abs() + Nk * 2.0 ** -24 * vmax
    if eps is not None:
        tol = tol + 2.0 * eps[..., None] * A
    return tol


def max_log2_score(qh, kh, scale=SCALE):
    return float(((qh @ kh.transpose(-1, -2)) * (scale * LOG2E)).abs().max())


def rope64(xh, pos, cos, sin):
    """RoPE2D in float64 from the fp32 tables.  xh [B,H,N,64] float64, pos
    [B,N,2] int64 (y, x), cos / sin [maxpos,16] fp32.  Head dims [0,32) turn
    with y, [32,64) with x; inside a half, dim d pairs with d+16."""
    out = torch.empty_like(xh)
    for half in range(2):
        p = pos[:, :, half]
        c = cos.double()[p][:, None]          # [B,1,N,16]
        s = sin.double()[p][:, None]
        a = xh[..., 32 * half:32 * half + 16]
        b = xh[..., 32 * half + 16:32 * half + 32]
        out[..., 32 * half:32 * half + 16] = a * c - b * s
        out[..., 32 * half + 16:32 * half + 32] = b * c + a * s
    return out


def rope_inputs(qh, kh, qpos, kpos, cos, sin):
    """Rotated Q and K rounded once to fp16 (as float64 again)."""
    return (rope64(qh, qpos, cos, sin).half().double(),
            rope64(kh, kpos, cos, sin).half().double())


def rope_eps(qr, kr, scale=SCALE):
    """eps_i of the module docstring, [B,H,Nq]."""
    return scale * 2.0 ** -10 * (qr.abs() @ kr.abs().transpose(-1, -2)).amax(-1)


def reference_rows(q, k, v, B, Nq, Nk, H, scale=SCALE, rope=None):
    """Row-layout front end: fp16 rows in, (ref, tol) [B*Nq, H*64] float64 out.
    rope = (qpos, kpos, cos, sin) selects the RoPE reference and bound."""
    qh, kh, vh = to_heads(q, B, Nq, H), to_heads(k, B, Nk, H), to_heads(v, B, Nk, H)
    eps = None
    if rope is not None:
        qh, kh = rope_inputs(qh, kh, *rope)
        eps = rope_eps(qh, kh, scale)
    ref, A = reference(qh, kh, vh, scale)
    return to_rows(ref), to_rows(tolerance(ref, A, vh, eps))


def worst(o, ref, tol, B, Nq, H):
    """Worst err / tol of o [G, B*Nq, H*64] and where: (ratio, (g, b, h, row, d)).
    A NaN anywhere counts as an infinite ratio."""
    ratio = (o.double() - ref).abs() / tol
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    flat = int(ratio.argmax())
    G, R, C = ratio.shape
    g, r, c = flat // (R * C), (flat // C) % R, flat % C
    return float(ratio.reshape(-1)[flat]), (g, r // Nq, c // D, r % Nq, c % D)


def f16_ordinal(x):
    """fp16 bits -> integers ordered like the values (for ulp distances)."""
    b = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7fff))


# ---------------------------------------------------------------- families ---
def onehot_targets(Nq, Nk, start, gen):
    """pi: key 0, key Nk-1 and both sides of every 16-key (so every 64-key)
    boundary, taken from `start` on so that small Nq still reach all of them
    over the heads; the rest random."""
    special = [0, Nk - 1]
    for e in range(16, Nk, 16):
        special += [e - 1, e]
    special = list(dict.fromkeys(special))
    pi = torch.randint(0, Nk, (Nq,), generator=gen)
    n = min(Nq, len(special))
    pi[:n] = torch.tensor([special[(start + i) % len(special)] for i in range(n)])
    return pi


def _unit(gen, *shape):
    u = torch.randn(*shape, D, generator=gen)
    return u / u.norm(dim=-1, keepdim=True)


def make_inputs(family, B, Nq, Nk, H, groups, seed=0, device="cpu"):
    """Per group (Q [B*Nq, H*64], K, V [B*Nk+SPARE, H*64]) fp16, seeded; every
    group, batch and head gets its own data."""
    assert family in FAMILIES, family
    out = []
    for g in range(groups):
        gen = torch.Generator().manual_seed(1000003 * seed + 7919 * g + FAMILIES.index(family))
        rn = lambda *s: torch.randn(*s, generator=gen)
        q, k, v = rn(B, H, Nq, D), rn(B, H, Nk, D), rn(B, H, Nk, D)
        ks, vs = rn(SPARE, H * D), rn(SPARE, H * D)
        if family == "random_q4":
            q = q * 4
        elif family in ("onehot8", "onehot32"):
            if family == "onehot32":
                # |k| = 8 keeps the matched score at 32 * 64 / 8 * log2 e = 369 <= 400
                k = k * (8 / k.norm(dim=-1, keepdim=True))
                k = k * (1 - 2.0 ** -9)          # fp16 rounding cannot push |k|^2 above 64
            k = k.half().float()
            f = 8.0 if family == "onehot8" else 32.0
            for b in range(B):
                for h in range(H):
                    pi = onehot_targets(Nq, Nk, ((g * B + b) * H + h) * Nq, gen)
                    q[b, h] = f * k[b, h, pi]
        elif family in ("ramp_up", "ramp_down"):
            u = _unit(gen, B, H, 1)
            t = torch.linspace(-8, 8, Nk)
            if family == "ramp_down":
                t = t.flip(0)
            k = t[None, None, :, None] * u + 0.1 * k
            q = 8 * u + 0.1 * q
        elif family == "uniform":
            q = torch.zeros_like(q)
        elif family == "allneg":
            u = _unit(gen, B, H, 1)
            c = 16 + torch.rand(B, H, Nk, 1, generator=gen)
            k = c * u + 0.1 * k
            q = -16 * u + 0.1 * q
        elif family == "intruder":
            ub = torch.linalg.qr(rn(D, B))[0].T          # [B, 64] orthonormal
            q = q + 4 * ub[:, None, None, :]
        Q, K, V = to_rows(q), torch.cat([to_rows(k), ks]), torch.cat([to_rows(v), vs])
        if family == "intruder":
            for b in range(B):          # the row behind batch b's keys
                K[(b + 1) * Nk] = (32 * ub[b]).repeat(H)
                V[(b + 1) * Nk] = 1000.0
        elif family == "nan":
            K[B * Nk:] = math.nan
            V[B * Nk:] = math.nan
        out.append(tuple(t.half().to(device) for t in (Q, K, V)))
    return out


# --------------------------------------------------------------- emulation ---
def emulate(q, k, v, scale=SCALE, split=2):
    """The kernels' arithmetic for one head, tile by tile: 64-key tiles, fp32
    scores and online softmax in base 2, P rounded to fp16, fp32 accumulation,
    `split` key groups (tiles sp, sp + split, ...) merged at the end, fp16
    output.  q [Nq,64], k / v [Nk,64] fp16 on the CPU."""
    sl = torch.tensor(scale * LOG2E, dtype=torch.float32)
    Nq, Nk = q.shape[0], k.shape[0]
    NT = (Nk + KT - 1) // KT
    qf = q.float()
    parts = []
    for sp in range(split):
        m = torch.full((Nq,), -math.inf)
        l = torch.zeros(Nq)
        o = torch.zeros(Nq, D)
        for t in range(sp, NT, split):
            kk, vv = k[t * KT:(t + 1) * KT].float(), v[t * KT:(t + 1) * KT].float()
            s = qf @ kk.T
            mn = torch.maximum(m, s.max(-1).values * sl)
            a = torch.exp2(m - mn)
            m = mn
            e = torch.exp2(s * sl - mn[:, None])
            l = l * a + e.sum(-1)
            o = o * a[:, None] + e.half().float() @ vv
        parts.append((m, l, o))
    m, l, o = parts[0]
    for m2, l2, o2 in parts[1:]:          # an idle group has m2 = -inf, l2 = 0
        mm = torch.maximum(m, m2)
        a1, a2 = torch.exp2(m - mm), torch.exp2(m2 - mm)
        l, o, m = l * a1 + l2 * a2, o * a1[:, None] + o2 * a2[:, None], mm
    return (o / l[:, None]).half()
