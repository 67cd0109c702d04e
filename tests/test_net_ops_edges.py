"""Every kernel of csrc/net_ops.hip (LayerNorm, bilinear x2 upsample,
Gaussian-head postprocess, fp32 -> fp16 cast, patch im2col, PRNG fill) against
the float64 references and the derived per-element bounds of
tests/net_ops_ref64.py, at the smallest shapes at which each can go wrong:
both column edges of every k_layernorm instantiation, last workgroups with
idle waves, groups, strided and column-slice layouts, NULL outputs, odd
output widths of the upsample under 1, 2 and 4 pixels per thread, crops,
1-pixel images, the postprocess's clips and cancellations, every fp16
rounding tie of the cast.

Every GPU test launches through the wrappers of splatt3r_amd/ops.py, prefills
its outputs with a NaN bit pattern no kernel produces and asserts bit for bit
that exactly the specified footprint was written.

S3_UPSAMPLE_PX is read once per process, so the 1- and 4-pixel kernels run in
one fresh child process each (the `__main__` entry at the bottom), one after
the other, and must reproduce this process's outputs bit for bit.

Not tested here: the int64_t index instantiations of k_upsample2x, which need
B oh ow C/8 >= 2^31, i.e. an output of at least 32 GiB.

The test_oracle_* tests need no GPU: they check the references against
torch's own float64 operators, that a plain fp32 emulation of each kernel
stays inside its bound on every family and shape the GPU tests use, and that
every deliberately wrong variant breaks it.
"""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net_ops_ref64 as R

gpu = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------- cases ---
LN_WIDTHS = (4, 8, 252, 256, 260, 512, 516, 768, 1024, 1028, 1280, 2048)
LN_ROWS = (1, 2, 3, 4, 5, 7, 37)
LN_GROUPS = (1, 2, 4)
LN_LAYOUTS = ("dense", "padded", "slice")
LN_OUTPUTS = ("both", "f32", "f16")
LN_SETTING_WIDTHS = (260, 768, 1028)
LN_WIDTH_ROWS, LN_WIDTH_GROUPS = 5, 2          # 5 rows: a last workgroup with three idle waves

PP_NS = (1, 255, 256, 257, 513)
PP_LDS = ((4, 14), (16, 16))


def ln_settings(C):
    """Every rows / groups / outputs combination with a family, cycling."""
    out = []
    for i, (rows, groups, outputs) in enumerate(itertools.product(LN_ROWS, LN_GROUPS, LN_OUTPUTS)):
        out.append((rows, groups, outputs, R.LN_FAMILIES[(i + C) % len(R.LN_FAMILIES)]))
    return out


def pp_settings():
    return list(itertools.product(PP_LDS, (0, 1), (False, True)))


# ----------------------------------------------------------------- helpers ---
def _sentinel(shape, dtype, device=DEV):
    t = torch.empty(shape, dtype=dtype, device=device)
    if dtype == torch.float32:
        t.view(torch.int32).fill_(R.SENT32)
    else:
        t.view(torch.int16).fill_(R.SENT16)
    return t


def _is_sentinel(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32) == R.SENT32
    return t.contiguous().view(torch.int16) == R.SENT16


def _assert_footprint(buf, mask, what):
    """Exactly the elements of `mask` were written."""
    s = _is_sentinel(buf).cpu()
    mask = mask.expand_as(s) if mask.shape != s.shape else mask
    assert bool(s[~mask].all()), f"{what}: wrote outside its footprint"
    assert not bool(s[mask].any()), f"{what}: left part of its footprint unwritten"


def _stream():
    from splatt3r_amd import _lib
    return _lib.stream()


# --------------------------------------------------------------- LayerNorm ---
def _ln_launch(inputs, rows, C, layout, outputs, eps=R.LN_EPS, launch=True):
    """One launch on fresh, sentinel-filled buffers; returns per group
    (o32 [rows, C] or None, o16 or None) on the CPU after the footprint check."""
    from splatt3r_amd import ops
    off = C if layout == "slice" else 0
    ldx = {"dense": C, "padded": C + 4, "slice": 3 * C}[layout]
    ld32 = {"dense": C, "padded": C + 8, "slice": C}[layout]
    ld16 = {"dense": C, "padded": C + 12, "slice": 3 * C}[layout]
    off16 = off
    xs, gs, bs, b32, b16 = [], [], [], [], []
    for x, g, b in inputs:
        xb = torch.full((rows + 1, ldx), math.nan)
        xb[:rows, off:off + C] = x
        xs.append(xb.to(DEV))
        gs.append(g.to(DEV))
        bs.append(b.to(DEV))
        b32.append(_sentinel((rows + 1, ld32), torch.float32))
        b16.append(_sentinel((rows + 1, ld16), torch.float16))
    want32, want16 = outputs in ("both", "f32"), outputs in ("both", "f16")
    call = ops.layernorm([x[:, off:] for x in xs], gs, bs, rows=rows, C=C, ldx=ldx, eps=eps,
                         out16=[o[:, off16:] for o in b16] if want16 else None, ld16=ld16 if want16 else 0,
                         out32=b32 if want32 else None, ld32=ld32 if want32 else 0)
    if not launch:
        return call, b32, b16
    call(_stream())
    torch.cuda.synchronize()
    out = []
    for g in range(len(inputs)):
        m32 = torch.zeros(rows + 1, ld32, dtype=torch.bool)
        m16 = torch.zeros(rows + 1, ld16, dtype=torch.bool)
        if want32:
            m32[:rows, :C] = True
        if want16:
            m16[:rows, off16:off16 + C] = True
        _assert_footprint(b32[g], m32, f"layernorm fp32 g{g}")
        _assert_footprint(b16[g], m16, f"layernorm fp16 g{g}")
        out.append((b32[g][:rows, :C].cpu() if want32 else None,
                    b16[g][:rows, off16:off16 + C].cpu() if want16 else None))
    return out


def _ln_worst(inputs, outs):
    """Worst err / bound of the fp32 and of the fp16 output over the groups,
    each group against its own reference."""
    w32 = w16 = 0.0
    for (x, g, b), (o32, o16) in zip(inputs, outs):
        y, t32, t16 = R.ln_reference(x, g, b)
        if o32 is not None:
            w32 = max(w32, R.worst_ratio(o32, y, t32))
        if o16 is not None:
            w16 = max(w16, R.worst_ratio(o16, y, t16))
    return w32, w16


@gpu
@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_every_width_and_family(C, parity):
    from splatt3r_amd import ops
    ops.f16_saturations(reset=True)
    for fam in R.LN_FAMILIES:
        inputs = R.ln_inputs(fam, LN_WIDTH_ROWS, C, LN_WIDTH_GROUPS, seed=C)
        outs = _ln_launch(inputs, LN_WIDTH_ROWS, C, "dense", "both")
        w32, w16 = _ln_worst(inputs, outs)
        parity(f"layernorm/{fam}/C{C}/f32", err=w32, tol=1.0)
        parity(f"layernorm/{fam}/C{C}/f16", err=w16, tol=1.0)
        assert max(w32, w16) <= 1.0, (fam, C, w32, w16)
    assert ops.f16_saturations() == 0


@gpu
@pytest.mark.parametrize("layout", LN_LAYOUTS)
@pytest.mark.parametrize("C", LN_SETTING_WIDTHS)
def test_layernorm_every_launch_setting(C, layout, parity):
    from splatt3r_amd import ops
    ops.f16_saturations(reset=True)
    worst = {}
    for rows, groups, outputs, fam in ln_settings(C):
        inputs = R.ln_inputs(fam, rows, C, groups, seed=rows)
        outs = _ln_launch(inputs, rows, C, layout, outputs)
        w = _ln_worst(inputs, outs)
        for kind, v in zip(("f32", "f16"), w):
            worst[fam, kind] = max(worst.get((fam, kind), 0.0), v)
        assert max(w) <= 1.0, (rows, groups, outputs, fam, w)
    for (fam, kind), v in worst.items():
        parity(f"layernorm/{fam}/C{C}/{layout}/{kind}", err=v, tol=1.0)
    assert ops.f16_saturations() == 0


@gpu
def test_layernorm_zero_rows_is_a_noop():
    inputs = R.ln_inputs("normal", 0, 260, 2)
    call, b32, b16 = _ln_launch(inputs, 0, 260, "dense", "both", launch=False)
    call(_stream())
    torch.cuda.synchronize()
    assert all(bool(_is_sentinel(b).all()) for b in b32 + b16)


@gpu
@pytest.mark.parametrize("what", ["C0", "C6", "C2052", "groups0", "groups5", "ldx"])
def test_layernorm_rejects_bad_arguments(what):
    from splatt3r_amd import ops
    rows, C, ld, groups = 3, 8, 2052, 1          # buffers as wide as the widest rejected C
    ldx = ld
    if what.startswith("C"):
        C = int(what[1:])
    elif what == "ldx":
        ldx = C + 2
    else:
        groups = int(what[6:])
    x = [torch.randn(rows + 1, ld, device=DEV) for _ in range(groups)]
    gb = [torch.randn(ld, device=DEV) for _ in range(groups)]
    b32 = [_sentinel((rows + 1, ld), torch.float32) for _ in range(groups)]
    b16 = [_sentinel((rows + 1, ld), torch.float16) for _ in range(groups)]
    # five groups do not fit the wrapper's pointer array: it raises before the library can
    with pytest.raises((RuntimeError, IndexError), match="s3n_layernorm|index"):
        ops.layernorm(x, gb, gb, rows=rows, C=C, ldx=ldx, out16=b16, ld16=ld, out32=b32,
                      ld32=ld)(_stream())
    torch.cuda.synchronize()
    assert all(bool(_is_sentinel(b).all()) for b in b32 + b16)


@gpu
def test_layernorm_fp16_output_saturates_where_fp32_does_not(parity):
    """gamma scaled until some |y| > 65504: the fp16 output is +-65504 exactly
    there, the fp32 output is not clamped, the flag is set and reset clears it."""
    from splatt3r_amd import ops
    ops.f16_saturations(reset=True)
    rows, C = 5, 260
    x, g, b = R.ln_inputs("normal", rows, C, 1)[0]
    g = g * 4e4
    (o32, o16), = _ln_launch([(x, g, b)], rows, C, "dense", "both")
    y, t32, _ = R.ln_reference(x, g, b)
    w = R.worst_ratio(o32, y, t32)
    parity("layernorm/saturating_gamma/C260/f32", err=w, tol=1.0)
    assert w <= 1.0
    over = o32.abs() > 65504.0
    assert bool(over.any()) and not bool(over.all())
    assert torch.equal(o16[over].float(), torch.copysign(torch.tensor(65504.0), o32[over]))
    assert torch.equal(o16[~over], o32[~over].half())
    assert ops.f16_saturations(reset=True) == 1
    assert ops.f16_saturations() == 0


# ---------------------------------------------------------------- upsample ---
def _up_launch(inputs, B, H, W, C, oh, ow):
    """Per group the [B, oh, ow, C] fp16 output on the CPU, footprint checked."""
    from splatt3r_amd import ops
    n = B * oh * ow * C
    xs = [x.to(DEV) for x in inputs]
    outs = [_sentinel((n + ow * C,), torch.float16) for _ in inputs]
    ops.upsample2x(xs, outs, B=B, H=H, W=W, C=C, oh=oh, ow=ow)(_stream())
    torch.cuda.synchronize()
    mask = torch.zeros(n + ow * C, dtype=torch.bool)
    mask[:n] = True
    for g, o in enumerate(outs):
        _assert_footprint(o, mask, f"upsample g{g}")
    return [o[:n].cpu().reshape(B, oh, ow, C) for o in outs]


def _up_case_outputs(case):
    fam, H, W, oh, ow, C, B, groups = case
    inputs = R.up_inputs(fam, B, H, W, C, groups, seed=H * 100 + W)
    return inputs, _up_launch(inputs, B, H, W, C, oh, ow)


@gpu
@pytest.mark.parametrize("case", R.up_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_upsample_edges(case, parity):
    fam, H, W, oh, ow, C, B, groups = case
    inputs, outs = _up_case_outputs(case)
    w = 0.0
    for x, o in zip(inputs, outs):
        ref, tol = R.up_reference(x, B, H, W, C, oh, ow)
        assert bool(torch.isfinite(o).all()), "a convex combination of finite pixels is finite"
        w = max(w, R.worst_ratio(o, ref, tol))
    parity(f"upsample/{fam}/{H}x{W}->{oh}x{ow}/C{C}B{B}g{groups}", err=w, tol=1.0)
    assert w <= 1.0, (case, w)


def _up_all_bits():
    return [[o.view(torch.int16) for o in _up_case_outputs(c)[1]] for c in R.up_cases()]


@gpu
def test_upsample_one_and_four_pixels_per_thread_match_two(tmp_path):
    assert os.environ.get("S3_UPSAMPLE_PX", "2")[:1] not in ("1", "4"), "this process must run PX=2"
    mine = _up_all_bits()
    for px in ("1", "4"):          # one after the other; a failing child stops the test
        path = str(tmp_path / f"px{px}.pt")
        env = dict(os.environ, S3_UPSAMPLE_PX=px)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--upsample-child", path],
                           env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, (px, r.stdout[-2000:], r.stderr[-2000:])
        theirs = torch.load(path)
        assert theirs["px"] == px and len(theirs["out"]) == len(mine)
        for case, a, b in zip(R.up_cases(), mine, theirs["out"]):
            for g, (oa, ob) in enumerate(zip(a, b)):
                assert torch.equal(oa, ob), (px, case, g)


# ------------------------------------------------------------- postprocess ---
def _pp_launch(n, pts, feat, gs, ld_pts, ld_g, use_offsets, with16):
    from splatt3r_amd import ops
    out = {k: _sentinel((n + 1, c), torch.float32) for k, c in R.PP_OUT.items()}
    d16 = _sentinel((n + 1, 24), torch.float16) if with16 else None
    ops.gaussian_postprocess(n, pts.to(DEV), ld_pts, feat.to(DEV), gs.to(DEV), ld_g, use_offsets, out,
                             desc16=d16)(_stream())
    torch.cuda.synchronize()
    mask = torch.zeros(n + 1, 1, dtype=torch.bool)
    mask[:n] = True
    for k, v in out.items():
        _assert_footprint(v, mask, f"postprocess {k}")
    res = {k: v[:n].cpu() for k, v in out.items()}
    if with16:
        _assert_footprint(d16, mask, "postprocess desc16")
        assert R.f16_equal(d16[:n].cpu(), res["desc"].half()), "desc16 is desc rounded to fp16"
    return res


@gpu
@pytest.mark.parametrize("family", R.PP_FAMILIES)
@pytest.mark.parametrize("n", PP_NS)
def test_postprocess_edges(n, family, parity):
    worst = dict.fromkeys(R.PP_OUT, 0.0)
    for (ld_pts, ld_g), use_offsets, with16 in pp_settings():
        pts, feat, gs = R.pp_inputs(family, n, ld_pts, ld_g, seed=n)
        got = _pp_launch(n, pts, feat, gs, ld_pts, ld_g, use_offsets, with16)
        ref = R.pp_reference(pts, feat, gs, use_offsets)
        if not use_offsets:
            assert torch.equal(got["means"].view(torch.int32), got["pts3d"].view(torch.int32))
        for k, (r, t) in ref.items():
            w = R.worst_ratio(got[k], r, t)
            worst[k] = max(worst[k], w)
            assert w <= 1.0, (k, n, family, ld_pts, ld_g, use_offsets, w)
    for k, w in worst.items():
        parity(f"postprocess/{family}/{k}/n{n}", err=w, tol=1.0)


# -------------------------------------------------------------------- cast ---
def _cast_launch(x, rows, cols, ld_in, ld_out, out_cols=None, out_off=0):
    """x [rows, cols] fp32 on the CPU -> the [rows, cols] fp16 result."""
    from splatt3r_amd import ops
    xin = torch.full((rows, ld_in), 1234.0)
    xin[:, :cols] = x
    buf = _sentinel((rows + 1, out_cols or ld_out), torch.float16)
    ops.cast_f16(xin.to(DEV), buf[:, out_off:], rows=rows, cols=cols, ld_in=ld_in,
                 ld_out=ld_out)(_stream())
    torch.cuda.synchronize()
    s = _is_sentinel(buf).cpu()
    mask = torch.zeros_like(s)
    mask[:rows, out_off:out_off + cols] = True
    assert bool(s[~mask].all()), "cast wrote outside its footprint"
    # the fp32 image of the sentinel NaN itself casts back to the sentinel
    assert not bool((s[:rows, out_off:out_off + cols] & ~x.isnan()).any()), "cast left elements unwritten"
    return buf[:rows, out_off:out_off + cols].cpu()


def _cast_pool():
    parts = [R.cast_values("edges")]
    for fam in ("midpoints", "subnormal", "f16_images"):
        v = R.cast_values(fam)
        parts.append(v[::max(1, v.numel() // 600)])
    return torch.cat(parts)


@gpu
@pytest.mark.parametrize("family", R.CAST_FAMILIES)
def test_cast_rounds_every_value_to_nearest_even(family):
    v = R.cast_values(family)
    cols = 256
    rows = -(-v.numel() // cols)
    x = v[torch.arange(rows * cols) % v.numel()].reshape(rows, cols)
    got = _cast_launch(x, rows, cols, cols, cols)
    assert R.f16_equal(got, x.half())


@gpu
@pytest.mark.parametrize("shape", R.CAST_SHAPES + ("slice",), ids=str)
def test_cast_layouts(shape):
    pool = _cast_pool()
    kw = {}
    if shape == "slice":          # destination: columns [64, 101) of an [8, 128] buffer
        shape, kw = (7, 37, 40, 128), dict(out_cols=128, out_off=64)
    rows, cols, ld_in, ld_out = shape
    x = pool[(torch.arange(rows * cols) * 7 + 3) % pool.numel()].reshape(rows, cols)
    if rows * cols == 1:
        x = torch.tensor([[65520.0]])          # no saturation: the tie above 65504 becomes inf
    got = _cast_launch(x, rows, cols, ld_in, ld_out, **kw)
    assert R.f16_equal(got, x.half())
    if rows * cols == 1:
        assert bool(torch.isinf(got).all())


# ------------------------------------------------------------------ im2col ---
@gpu
@pytest.mark.parametrize("family", ["index", "random"])
@pytest.mark.parametrize("B,H,W,p", R.IM2COL_SHAPES)
def test_im2col_bitexact(B, H, W, p, family):
    from splatt3r_amd import ops
    img = R.im2col_inputs(B, H, W, p, family)
    ref = R.im2col_reference(img, p)
    K = 3 * p * p
    A = _sentinel((ref.shape[0] + 1, K), torch.float16)
    ops.patch_im2col(img.to(DEV), A, B=B, H=H, W=W, p=p)(_stream())
    torch.cuda.synchronize()
    mask = torch.zeros(ref.shape[0] + 1, 1, dtype=torch.bool)
    mask[:-1] = True
    _assert_footprint(A, mask, "im2col")
    assert torch.equal(A[:-1].cpu().view(torch.int16), ref.view(torch.int16))


@gpu
def test_im2col_rejects_sizes_that_are_no_multiple_of_the_patch():
    from splatt3r_amd import ops
    img = R.im2col_inputs(1, 18, 16, 16).to(DEV)
    A = _sentinel((2, 768), torch.float16)
    with pytest.raises(RuntimeError, match="s3n_patch_im2col"):
        ops.patch_im2col(img, A, B=1, H=18, W=16, p=16)(_stream())
    torch.cuda.synchronize()
    assert bool(_is_sentinel(A).all())


# -------------------------------------------------------------------- PRNG ---
def _prng_seeds():
    from splatt3r_amd.weights import tensor_seed
    return (0, 1 << 63, (1 << 64) - 1, tensor_seed(1234, "enc_blocks.0.attn.qkv.weight"))


@gpu
@pytest.mark.parametrize("n", (0,) + R.PRNG_NS)
def test_prng_fill_bitexact(n):
    from splatt3r_amd import ops
    for seed in _prng_seeds():
        for a, c in R.PRNG_AC:
            buf = _sentinel((n + 8,), torch.float32)
            ops.prng_fill(buf[:n], seed, a, c)
            torch.cuda.synchronize()
            mask = torch.zeros(n + 8, dtype=torch.bool)
            mask[:n] = True
            _assert_footprint(buf, mask, "prng_fill")
            ref = R.prng_reference(seed, n, a, c)
            np.testing.assert_array_equal(buf[:n].cpu().numpy().view(np.int32), ref.view(np.int32))


# ============================================================ CPU oracles ====
def _ln_oracle_cases():
    for C in LN_WIDTHS:
        for fam in R.LN_FAMILIES:
            yield fam, LN_WIDTH_ROWS, C, LN_WIDTH_GROUPS, C
    for C in LN_SETTING_WIDTHS:
        for rows, groups, _, fam in ln_settings(C):
            yield fam, rows, C, groups, rows


def _ln_emulation_worst(wrong=None):
    worst = {}
    for fam, rows, C, groups, seed in _ln_oracle_cases():
        inputs = R.ln_inputs(fam, rows, C, groups, seed=seed)
        w = _ln_worst(inputs, R.ln_emulate(inputs, wrong=wrong))
        for kind, v in zip(("f32", "f16"), w):
            worst[fam, kind] = max(worst.get((fam, kind), 0.0), v)
    return worst


def _up_emulation_worst(wrong=None, only=lambda H, W, oh, ow: True):
    worst = {}
    for fam, H, W, oh, ow, C, B, groups in R.up_cases():
        if not only(H, W, oh, ow):
            continue
        for x in R.up_inputs(fam, B, H, W, C, groups, seed=H * 100 + W):
            ref, tol = R.up_reference(x, B, H, W, C, oh, ow)
            w = R.worst_ratio(R.up_emulate(x, B, H, W, C, oh, ow, wrong=wrong), ref, tol)
            worst[fam] = max(worst.get(fam, 0.0), w)
    return worst


def _pp_emulation_worst(wrong=None):
    worst = {}
    for n in PP_NS:
        for fam in R.PP_FAMILIES:
            for (ld_pts, ld_g), use_offsets, _ in pp_settings()[::2]:
                pts, feat, gs = R.pp_inputs(fam, n, ld_pts, ld_g, seed=n)
                got = R.pp_emulate(pts, feat, gs, use_offsets, wrong=wrong)
                for k, (r, t) in R.pp_reference(pts, feat, gs, use_offsets).items():
                    w = R.worst_ratio(got[k].reshape(r.shape), r, t)
                    worst[fam, k] = max(worst.get((fam, k), 0.0), w)
    return worst


def test_oracle_references_agree_with_torch_float64():
    for C in (4, 260, 2048):
        x, g, b = R.ln_inputs("offset1000", 5, C, 1)[0]
        y, _, _ = R.ln_reference(x, g, b)
        t = F.layer_norm(x.double(), (C,), g.double(), b.double(), eps=float(np.float32(R.LN_EPS)))
        assert float((y - t).abs().max()) <= 1e-12 * float(t.abs().max())
    for H, W, oh, ow in R.UP_SHAPES:
        x = R.up_inputs("random", 2, H, W, 8, 1)[0]
        ref, _ = R.up_reference(x, 2, H, W, 8, oh, ow)
        img = x[:2 * H * W * 8].reshape(2, H, W, 8).double().permute(0, 3, 1, 2)
        t = F.interpolate(img, scale_factor=2, mode="bilinear", align_corners=True)
        t = t[:, :, :oh, :ow].permute(0, 2, 3, 1)
        assert float((ref - t).abs().max()) <= 1e-12
    for B, H, W, p in R.IM2COL_SHAPES:
        for fam in ("index", "random"):
            img = R.im2col_inputs(B, H, W, p, fam)
            t = F.unfold(img.half().float(), p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p).half()
            assert torch.equal(R.im2col_reference(img, p).view(torch.int16), t.view(torch.int16))
        if B * 3 * H * W <= 4097:
            assert R.im2col_inputs(B, H, W, p).unique().numel() == B * 3 * H * W
        assert float(R.im2col_inputs(B, H, W, p).abs().max()) <= 2048
    # the cast's reference against numpy's own converter
    for fam in R.CAST_FAMILIES:
        v = R.cast_values(fam)
        with np.errstate(over="ignore"):
            assert R.f16_equal(v.half(), torch.from_numpy(v.numpy().astype(np.float16)))
    assert R.cast_values("f16_images").numel() == 65536
    # postprocess: the same formulas once more, written directly
    pts, feat, gs = R.pp_inputs("normal", 257, 16, 16)
    ref = R.pp_reference(pts, feat, gs, 1)
    P, Fe, G = pts.double(), feat.double(), gs.double()
    d = P[:, :3].norm(dim=-1, keepdim=True)
    od = G[:, :3].norm(dim=-1, keepdim=True)
    p3 = P[:, :3] / d * torch.expm1(d)
    direct = dict(pts3d=p3, means=p3 + G[:, :3] / od * ((od - 6).exp() - math.exp(-6)),
                  opacities=torch.sigmoid(G[:, 13]), conf=1 + P[:, 3].exp(),
                  rotations=G[:, 6:10] / (G[:, 6:10].norm(dim=-1, keepdim=True) + R.CLIP),
                  desc=F.normalize(Fe[:, :24], dim=-1), scales=G[:, 3:6].exp())
    for k, v in direct.items():
        assert float(((ref[k][0] - v).abs() / v.abs().clamp(min=1e-3)).max()) <= 1e-12, k


def test_oracle_families_are_what_they_claim():
    for fam in R.UP_FAMILIES:
        x = R.up_inputs(fam, 3, 12, 16, 16, 4)
        for g, t in enumerate(x):
            body = t[:3 * 12 * 16 * 16]
            assert bool(torch.isfinite(body).all()) and bool(t[body.numel():].isnan().all())
            if fam == "subnormal":
                assert bool(((body.abs() > 0) & (body.abs() < 2.0 ** -14)).all())
            if fam == "index":      # the value identifies (b, y, x, c mod 8)
                assert body.reshape(-1, 16)[:, :8].unique().numel() == 3 * 12 * 16 * 8
    for n in PP_NS:
        pts, feat, gs = R.pp_inputs("descnorm", n, 4, 14)
        assert int((feat[:, :24] == 0).all(-1).sum()) == 1
        pts, _, gs = R.pp_inputs("small", n, 4, 14)
        assert bool((pts[:, :3] == 0).all(-1).any()) and bool((gs[:, :3] == 0).all(-1).any())
    # inputs stay where fp32 sums of squares neither overflow nor vanish (zero
    # rows apart): a single square flushed to zero is below 2^-24 of its row's sum
    for fam in R.PP_FAMILIES:
        pts, feat, gs = R.pp_inputs(fam, 513, 4, 14)
        for v in (pts[:, :3], feat[:, :24], gs[:, :3], gs[:, 6:10]):
            ss = (v * v).sum(-1)
            ss = ss[(v != 0).any(-1)]
            assert bool(torch.isfinite(ss).all()) and bool((ss >= 2.0 ** -102).all())


def test_oracle_prng_restatement_matches_the_numpy_twin():
    from splatt3r_amd.weights import prng_numpy, tensor_seed
    seeds = (0, 1 << 63, (1 << 64) - 1, tensor_seed(1234, "enc_blocks.0.attn.qkv.weight"))
    for seed in seeds:
        for a, c in R.PRNG_AC:
            np.testing.assert_array_equal(R.prng_reference(seed, 257, a, c).view(np.int32),
                                          prng_numpy(seed, 257, a, c).view(np.int32))


def test_oracle_emulations_stay_inside_the_bounds():
    ln, up, pp = _ln_emulation_worst(), _up_emulation_worst(), _pp_emulation_worst()
    print("layernorm", {k: round(v, 3) for k, v in ln.items()})
    print("upsample", {k: round(v, 3) for k, v in up.items()})
    per_out = {}
    for (fam, k), v in pp.items():
        per_out[k] = max(per_out.get(k, 0.0), v)
    print("postprocess", {k: round(v, 3) for k, v in per_out.items()})
    assert max(ln.values()) <= 1.0, ln
    assert max(up.values()) <= 1.0, up
    assert max(pp.values()) <= 1.0, pp
    assert {k[0] for k in ln} == set(R.LN_FAMILIES) and set(up) == set(R.UP_FAMILIES)


@pytest.mark.parametrize("wrong", R.LN_WRONG)
def test_oracle_wrong_layernorm_breaks_the_bound(wrong):
    w = _ln_emulation_worst(wrong)
    print(wrong, {k: round(v, 2) for k, v in w.items()})
    assert max(w.values()) > 1.0, w
    if wrong == "no_eps":
        assert w["constant", "f32"] > 1.0, w
    if wrong == "one_pass":
        assert w["offset1000", "f32"] > 1.0 and w["offset3e4", "f32"] > 1.0, w


@pytest.mark.parametrize("wrong", R.UP_WRONG)
def test_oracle_wrong_upsample_breaks_the_bound(wrong):
    w = _up_emulation_worst(wrong)
    print(wrong, {k: round(v, 2) for k, v in w.items()})
    assert max(w.values()) > 1.0, w
    # where each one shows: the crop's scale on cropped shapes only, the skipped
    # tail on odd widths only, the missing clamp where the grid reaches the last
    # row or column (a 1-pixel axis always does)
    hidden = {"scale_from_crop": lambda H, W, oh, ow: (oh, ow) == (2 * H, 2 * W),
              "skip_tail": lambda H, W, oh, ow: ow % 2 == 0,
              "no_clamp": lambda H, W, oh, ow: 1 < H and 1 < W and oh < 2 * H and ow < 2 * W
              }.get(wrong)
    if hidden is not None:
        assert max(_up_emulation_worst(wrong, hidden).values()) <= 1.0
        shown = _up_emulation_worst(wrong, lambda *a: not hidden(*a))
        assert min(shown.values()) > 1.0, shown


@pytest.mark.parametrize("wrong", R.PP_WRONG)
def test_oracle_wrong_postprocess_breaks_the_bound(wrong):
    w = _pp_emulation_worst(wrong)
    broken = {k: v for k, v in w.items() if v > 1.0}
    print(wrong, {k: round(v, 2) for k, v in broken.items()})
    assert broken, w
    field = {"exp_minus_1": "pts3d", "no_clip": "pts3d", "no_quat_eps": "rotations",
             "offsets_ignored": "means"}[wrong]
    assert any(k[1] == field for k in broken), broken
    fam = {"exp_minus_1": "small", "no_clip": "small", "no_quat_eps": "quat"}.get(wrong)
    assert fam is None or any(k[0] == fam for k in broken), broken


def test_oracle_wrong_cast_and_im2col_differ():
    for fam in ("midpoints", "edges"):
        v = R.cast_values(fam)
        assert not R.f16_equal(R.cast_truncate(v), v.half())
    exact = R.cast_values("f16_images")
    assert R.f16_equal(R.cast_truncate(exact), exact.half())
    for B, H, W, p in R.IM2COL_SHAPES:
        img = R.im2col_inputs(B, H, W, p)
        ref = R.im2col_reference(img, p)
        for wrong in R.IM2COL_WRONG:
            if p > 1:
                assert not torch.equal(R.im2col_reference(img, p, wrong), ref), (wrong, B, H, W, p)


# ===================================================== upsample child entry ===
if __name__ == "__main__":
    # python tests/test_net_ops_edges.py --upsample-child OUT: every upsample
    # case under this process's S3_UPSAMPLE_PX, output bits saved to OUT
    assert len(sys.argv) == 3 and sys.argv[1] == "--upsample-child", sys.argv
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_repo, os.path.join(_repo, "splatt3r-slam_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    torch.save({"px": os.environ.get("S3_UPSAMPLE_PX", "2"), "out": _up_all_bits()}, sys.argv[2])
