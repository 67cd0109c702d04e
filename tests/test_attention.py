"""Every attention kernel of csrc/net_attn.hip against the float64 reference
and the derived per-element bound of tests/attention_ref64.py, at the tile
edges of the key rings and of the query workgroups, plus the structural
properties the kernels rely on (store footprint, workgroup order, row / head
independence, repeatability, host argument checks).

Kernels: the RoPE kernel k_attn (selected by passing positions; self and
cross positions) and the six kernels for pre-rotated q / k, selected with
s3n_attention_set_variant: 1 = k_attn_dma, 2 = k_attn_st<4,1,4>,
3 = k_attn_st<4,4,2>, 0 = k_attn_st<4,2,2> (the default), 4 = k_attn_st<2,2,2>,
5 = k_attn_st<8,2,2>.

The test_oracle_* tests need no GPU: they check the reference itself.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import attention_ref64 as R
from attention_ref64 import D, SCALE, SPARE

gpu = pytest.mark.gpu

NKS = (1, 17, 63, 64, 65, 128, 129, 191, 193, 256, 257, 320, 321, 513, 577, 641)
NQS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
BS, HS, GS = (1, 2, 3), (1, 3, 5), (1, 2, 4)


def _pairs():
    """Every Nk with two Nq, every Nq with at least two Nk, then a few chosen
    ones: several workgroups against many tiles and uneven splits."""
    pq = []
    for i, nk in enumerate(NKS):
        pq += [(NQS[(2 * i) % len(NQS)], nk), (NQS[(2 * i + 1) % len(NQS)], nk)]
    pq += [(200, 641), (129, 321), (65, 65), (1, 641)]
    out = []
    for i, (nq, nk) in enumerate(pq):
        out.append((nq, nk, BS[i % 3], HS[(i + i // 3) % 3], GS[(i + i // 9) % 3]))
    out[32] = (200, 641, 3, 5, 4)          # the largest case: every limit at once
    return out


PAIRS = _pairs()
ROPE_KERNELS = ("rope_self", "rope_cross")
VARIANTS = (1, 2, 3, 0, 4, 5)
KERNELS = ROPE_KERNELS + tuple(f"v{v}" for v in VARIANTS)
QTILE = {"rope_self": 64, "rope_cross": 64, "v1": 64, "v2": 64, "v3": 64, "v0": 64, "v4": 32,
         "v5": 128}
MAXPOS = 64
DEV = "cuda"
# an fp16 NaN no kernel produces: unwritten output is recognisable bit for bit
SENTINEL = 0x7E5A


# ----------------------------------------------------------------- helpers ---
def _positions(B, Nq, Nk, groups, cross, device):
    """(y, x) of a 32-wide token grid, every entry strictly below MAXPOS; the
    groups are shifted against each other, cross flips the key order."""
    n = max(Nq, Nk)
    idx = torch.arange(n, device=device)
    qpos, kpos = [], []
    for g in range(groups):
        base = torch.stack([idx // 32 + g, idx % 32 + 2 * g], -1)
        base = base[None].expand(B, -1, 2).to(torch.int64)
        qpos.append(base[:, :Nq].contiguous())
        kpos.append((base.flip(1) if cross else base)[:, :Nk].contiguous())
        assert int(base.max()) < MAXPOS
    return qpos, kpos


_TABLES = {}


def _tables(device):
    from splatt3r_amd.net import rope_tables
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = rope_tables(MAXPOS, device)
    return _TABLES[key]


def _strided(inputs, B, Nq, Nk, H, nan_spare):
    """The fused-QKV layout: one [rows, 3*H*64] buffer per group, q / k / v are
    column slices with row stride 3*H*64."""
    out = []
    HD = H * D
    for q, k, v in inputs:
        rows = max(B * Nq, B * Nk + SPARE)
        buf = torch.randn(rows, 3 * HD, device=q.device,
                          generator=torch.Generator(device=q.device).manual_seed(5)).half()
        if nan_spare:
            buf[B * Nk:, HD:] = float("nan")
        buf[:B * Nq, :HD] = q
        buf[:B * Nk + SPARE, HD:2 * HD] = k
        buf[:B * Nk + SPARE, 2 * HD:] = v
        out.append((buf[:, :HD], buf[:, HD:2 * HD], buf[:, 2 * HD:]))
    return out


def _new_out(groups, rows, cols, device):
    o = torch.empty(groups, rows, cols, device=device, dtype=torch.float16)
    o.view(torch.int16).fill_(SENTINEL)
    return o


def _launch(kernel, inputs, O, B, Nq, Nk, H, stride, o_stride=None, pos=None, xcd=True):
    """One s3n_attention launch of `kernel` on per-group (q, k, v) into O[g]."""
    from splatt3r_amd import ops, _lib
    L = _lib.lib()
    kw = {}
    if kernel in ROPE_KERNELS:
        kw = dict(qpos=pos[0], kpos=pos[1], rope=_tables(O.device))
    try:
        if kernel not in ROPE_KERNELS:
            L.s3n_attention_set_variant(int(kernel[1:]))
        L.s3n_attention_set_variant(-2 if xcd else -1)
        ops.attention([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs],
                      list(O), B=B, Nq=Nq, Nk=Nk, H=H, q_stride=stride, k_stride=stride,
                      v_stride=stride, o_stride=o_stride or H * D, scale=SCALE,
                      **kw)(_lib.stream())
    finally:
        L.s3n_attention_set_variant(0)
        L.s3n_attention_set_variant(-2)


def _refs(inputs, B, Nq, Nk, H, pos=None):
    """Stacked (ref, tol) [G, B*Nq, H*64] of the groups."""
    rt = []
    for g, (q, k, v) in enumerate(inputs):
        rope = None if pos is None else (pos[0][g], pos[1][g]) + tuple(_tables(q.device))
        rt.append(R.reference_rows(q, k, v, B, Nq, Nk, H, rope=rope))
    return torch.stack([r for r, _ in rt]), torch.stack([t for _, t in rt])


def _case(family, B, Nq, Nk, H, groups, seed):
    """Inputs, positions and the three references (no RoPE, self, cross)."""
    inputs = R.make_inputs(family, B, Nq, Nk, H, groups, seed=seed, device=DEV)
    pos = {k: _positions(B, Nq, Nk, groups, k == "rope_cross", DEV) for k in ROPE_KERNELS}
    refs = {None: _refs(inputs, B, Nq, Nk, H)}
    for k in ROPE_KERNELS:
        refs[k] = _refs(inputs, B, Nq, Nk, H, pos[k])
    return inputs, pos, refs


# worst measured err / tol per (kernel, family, tile count), reported by the last test
HEADROOM = {}


# ------------------------------------------------------------ oracle (CPU) ---
def test_oracle_reference_equals_sdpa_fp64():
    B, Nq, Nk, H = 2, 33, 129, 3
    (q, k, v), = R.make_inputs("random", B, Nq, Nk, H, 1, seed=1)
    qh, kh, vh = R.to_heads(q, B, Nq, H), R.to_heads(k, B, Nk, H), R.to_heads(v, B, Nk, H)
    ref, A = R.reference(qh, kh, vh)
    sd = F.scaled_dot_product_attention(qh, kh, vh, scale=SCALE)
    assert float((ref - sd).abs().max()) < 1e-13
    sa = F.scaled_dot_product_attention(qh, kh, vh.abs(), scale=SCALE)
    assert float((A - sa).abs().max()) < 1e-13
    rows, tol = R.reference_rows(q, k, v, B, Nq, Nk, H)
    assert torch.equal(rows.view(B, Nq, H, D).permute(0, 2, 1, 3), ref)
    assert float(tol.min()) > 0


def test_oracle_rope64_equals_rope_ref():
    from test_net_ops import rope_ref
    from splatt3r_amd.net import rope_tables
    B, N, H = 2, 70, 3
    cos, sin = rope_tables(MAXPOS, "cpu")
    qpos, kpos = _positions(B, N, N, 2, True, "cpu")
    x = torch.randn(B, H, N, D, generator=torch.Generator().manual_seed(2)).half()
    for pos in (qpos[1], kpos[1]):
        got = R.rope64(x.double(), pos, cos, sin)
        want = rope_ref(x.float(), pos, cos, sin)
        # rope_ref: two fp32 products and their sum, |x| < 8: below 2^-20
        assert float((got - want.double()).abs().max()) < 2.0 ** -20
    # zero position is the identity, so the rotation is applied to the right dims
    z = torch.zeros_like(qpos[0])
    assert torch.equal(R.rope64(x.double(), z, cos, sin), x.double())


def test_oracle_families_are_what_they_claim():
    B, Nq, Nk, H = 3, 40, 129, 2
    for fam in R.FAMILIES:
        (q, k, v), = R.make_inputs(fam, B, Nq, Nk, H, 1, seed=3)
        assert q.shape == (B * Nq, H * D) and k.shape == v.shape == (B * Nk + SPARE, H * D)
        qh, kh, vh = R.to_heads(q, B, Nq, H), R.to_heads(k, B, Nk, H), R.to_heads(v, B, Nk, H)
        assert R.max_log2_score(qh, kh) <= 400, fam
        assert bool(torch.isfinite(torch.stack([kh, vh])).all()), fam
        s2 = (qh @ kh.transpose(-1, -2)) * (SCALE * R.LOG2E)
        if fam == "allneg":
            assert float(s2.max()) <= -40
        if fam in ("onehot8", "onehot32"):
            top = s2.topk(2, -1).values
            margin = float((top[..., 0] - top[..., 1]).min())
            assert margin > (126 if fam == "onehot32" else 30), (fam, margin)
        if fam == "ramp_up":
            assert bool((s2[..., -1] > s2[..., 0] + 10).all())
        if fam == "intruder":
            # the row behind batch b's keys, read as one more key of batch b,
            # would move every row of that batch far outside the bound
            assert float(v[Nk].min()) == 1000
            ref, tol = R.reference_rows(q, k, v, 1, Nq, Nk, H)
            leak = R.reference_rows(q, k, v, 1, Nq, Nk + 1, H)[0]
            assert float(((leak - ref).abs() / tol).amax(1).min()) > 100
        if fam == "nan":
            assert bool(torch.isnan(k[B * Nk:]).all() and torch.isnan(v[B * Nk:]).all())
    pi = R.onehot_targets(200, 641, 0, torch.Generator().manual_seed(0))
    assert {0, 640, 15, 16, 63, 64, 575, 576, 639, 640} <= set(pi.tolist())


@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_emulation_within_tolerance(family):
    """The kernels' arithmetic, emulated tile by tile on the CPU, respects the
    derived bound: the reference and the bound agree with each other."""
    Nq = 70
    for Nk in (65, 129, 330, 577):
        (q, k, v), = R.make_inputs(family, 1, Nq, Nk, 1, 1, seed=4)
        ref, tol = R.reference_rows(q, k, v, 1, Nq, Nk, 1)
        for split in (1, 2, 4):
            o = R.emulate(q, k[:Nk], v[:Nk], split=split)
            if family == "uniform":
                d = (R.f16_ordinal(o) - R.f16_ordinal(ref.half())).abs()
                assert int(d.max()) <= 1, (Nk, split)
            ratio, at = R.worst(o[None], ref[None], tol[None], 1, Nq, 1)
            assert ratio <= 1.0, (family, Nk, split, ratio, at)


def test_oracle_bound_sees_one_leaked_or_lost_key():
    """A zero-filled key Nk entering the softmax, or key Nk-1 missing, is
    outside the check of the families built to show it (on random data the
    leak is inside the bound: that is what allneg and uniform are for)."""
    Nq, Nk = 40, 577
    for fam, leak, lost in (("allneg", True, True), ("uniform", True, True),
                            ("onehot8", False, True), ("random", False, True)):
        (q, k, v), = R.make_inputs(fam, 1, Nq, Nk, 1, 1, seed=5)
        ref, tol = R.reference_rows(q, k, v, 1, Nq, Nk, 1)
        kz, vz = k[:Nk + 1].clone(), v[:Nk + 1].clone()
        kz[Nk], vz[Nk] = 0, 0
        o_leak = R.reference_rows(q, kz, vz, 1, Nq, Nk + 1, 1)[0]
        o_lost = R.reference_rows(q, k, v, 1, Nq, Nk - 1, 1)[0]
        for on, o in ((leak, o_leak), (lost, o_lost)):
            if not on:
                continue
            if fam == "uniform":
                d = (R.f16_ordinal(o.half()) - R.f16_ordinal(ref.half())).abs()
                assert int(d.max()) >= 3, fam
            else:
                assert float(((o - ref).abs() / tol).max()) > 2, fam


# ---------------------------------------------------- kernels vs reference ---
@gpu
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("Nq,Nk,B,H,groups", PAIRS)
def test_kernels_vs_ref64(Nq, Nk, B, H, groups, family):
    """All eight kernel selections, dense and fused-QKV layouts, on one
    (shape, family): |o - ref| <= tol on every element (uniform: one fp16 ulp
    of fp16(ref) as well)."""
    inputs, pos, refs = _case(family, B, Nq, Nk, H, groups, seed=Nq * 1000 + Nk)
    layouts = (("dense", inputs, H * D),
               ("qkv", _strided(inputs, B, Nq, Nk, H, family == "nan"), 3 * H * D))
    bad = []
    for kernel in KERNELS:
        ref, tol = refs[kernel if kernel in ROPE_KERNELS else None]
        for lname, lin, stride in layouts:
            O = _new_out(groups, B * Nq, H * D, DEV)
            _launch(kernel, lin, O, B, Nq, Nk, H, stride, pos=pos.get(kernel))
            ratio, at = R.worst(O, ref, tol, B, Nq, H)
            key = (kernel, family, "1-2 key tiles" if Nk <= 128 else "3+ key tiles")
            HEADROOM[key] = max(HEADROOM.get(key, 0.0), ratio)
            if not ratio <= 1.0:
                bad.append(f"{kernel}/{lname}: err/tol {ratio:.3g} at (g,b,h,row,d)={at}")
            if family == "uniform":
                ulps = int((R.f16_ordinal(O) - R.f16_ordinal(ref.half())).abs().max())
                if ulps > 1:
                    bad.append(f"{kernel}/{lname}: {ulps} fp16 ulp from the mean of V")
    assert not bad, "\n".join(bad)


# -------------------------------------------------------- structural checks ---
def _footprint(O, B, Nq, H):
    """O [G, B*Nq + 8, H*64 + 64] pre-filled with the sentinel: padding
    columns and spare rows untouched, no sentinel left in the valid region."""
    bits = O.view(torch.int16)
    assert bool((bits[:, B * Nq:] == SENTINEL).all()), "a store landed in the spare rows"
    assert bool((bits[:, :, H * D:] == SENTINEL).all()), "a store landed in the padding columns"
    left = int((bits[:, :B * Nq, :H * D] == SENTINEL).sum())
    assert left == 0, f"{left} valid elements were never written"


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_store_footprint(kernel):
    for Nq, Nk, B, H, groups in ((1, 65, 1, 1, 1), (33, 129, 2, 3, 2), (65, 63, 3, 1, 4),
                                 (129, 193, 1, 5, 1), (200, 17, 2, 1, 2)):
        inputs = R.make_inputs("random", B, Nq, Nk, H, groups, seed=11, device=DEV)
        pos = _positions(B, Nq, Nk, groups, kernel == "rope_cross", DEV)
        O = _new_out(groups, B * Nq + 8, H * D + 64, DEV)
        _launch(kernel, inputs, O, B, Nq, Nk, H, H * D, o_stride=H * D + 64, pos=pos)
        _footprint(O, B, Nq, H)


# total workgroups -> (query tiles, B, H, groups); 7 and 17 are prime, so the
# head count carries them (the only shapes here with more than 5 heads)
WG_COUNTS = {1: (1, 1, 1, 1), 3: (1, 3, 1, 1), 7: (1, 1, 7, 1), 8: (2, 2, 1, 2), 9: (1, 3, 3, 1),
             15: (1, 3, 5, 1), 17: (1, 1, 17, 1), 30: (2, 3, 5, 1)}


@gpu
@pytest.mark.parametrize("total", sorted(WG_COUNTS))
@pytest.mark.parametrize("kernel", ("v2", "v3", "v0", "v4", "v5"))
def test_workgroup_order(kernel, total):
    """XCD-aware order on and off: the same bits, every tile written once."""
    shapes = [WG_COUNTS[total]]
    if kernel == "v4" and total == 7:
        shapes.append((7, 1, 1, 1))          # 7 query tiles of 32 rows
    for nqt, B, H, groups in shapes:
        Nq = min(nqt * QTILE[kernel] - 3, 200)
        assert -(-Nq // QTILE[kernel]) * B * H * groups == total
        Nk = 129
        inputs = R.make_inputs("random", B, Nq, Nk, H, groups, seed=12, device=DEV)
        ref, tol = _refs(inputs, B, Nq, Nk, H)
        outs = []
        for xcd in (True, False):
            O = _new_out(groups, B * Nq + 8, H * D + 64, DEV)
            _launch(kernel, inputs, O, B, Nq, Nk, H, H * D, o_stride=H * D + 64, xcd=xcd)
            _footprint(O, B, Nq, H)
            outs.append(O)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        ratio, at = R.worst(outs[0][:, :B * Nq, :H * D], ref, tol, B, Nq, H)
        assert ratio <= 1.0, (ratio, at)


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_row_independence(kernel):
    """Row i is the same bits whether 33, 65 or 129 query rows are computed."""
    Nk, H = 193, 1
    (q, k, v), = R.make_inputs("random_q4", 1, 129, Nk, H, 1, seed=13, device=DEV)
    qpos, kpos = _positions(1, 129, Nk, 1, kernel == "rope_cross", DEV)
    outs = []
    for Nq in (33, 65, 129):
        O = _new_out(1, Nq, H * D, DEV)
        _launch(kernel, [(q[:Nq].contiguous(), k, v)], O, 1, Nq, Nk, H, H * D,
                pos=([qpos[0][:, :Nq].contiguous()], kpos))
        outs.append(O.view(torch.int16)[0])
    assert torch.equal(outs[0], outs[1][:33])
    assert torch.equal(outs[1], outs[2][:65])


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_head_independence(kernel):
    """A (group, batch, head) slice run alone (B = H = groups = 1) gives the
    bits it gives inside B = 3, H = 5, groups = 4."""
    B, H, groups, Nq, Nk = 3, 5, 4, 65, 257
    inputs = R.make_inputs("random_q4", B, Nq, Nk, H, groups, seed=14, device=DEV)
    pos = _positions(B, Nq, Nk, groups, kernel == "rope_cross", DEV)
    O = _new_out(groups, B * Nq, H * D, DEV)
    _launch(kernel, inputs, O, B, Nq, Nk, H, H * D, pos=pos)
    for g, b, h in ((0, 0, 0), (1, 2, 3), (3, 1, 4), (3, 2, 4)):
        q, k, v = inputs[g]
        one = (q[b * Nq:(b + 1) * Nq, h * D:(h + 1) * D].contiguous(),
               k[b * Nk:(b + 1) * Nk, h * D:(h + 1) * D].contiguous(),
               v[b * Nk:(b + 1) * Nk, h * D:(h + 1) * D].contiguous())
        o1 = _new_out(1, Nq, D, DEV)
        _launch(kernel, [one], o1, 1, Nq, Nk, 1, D,
                pos=([pos[0][g][b:b + 1].contiguous()], [pos[1][g][b:b + 1].contiguous()]))
        want = O[g, b * Nq:(b + 1) * Nq, h * D:(h + 1) * D]
        assert torch.equal(o1[0].view(torch.int16), want.contiguous().view(torch.int16)), (g, b, h)


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_repeatability(kernel):
    B, H, groups, Nq, Nk = 2, 3, 2, 129, 577
    inputs = R.make_inputs("random", B, Nq, Nk, H, groups, seed=15, device=DEV)
    pos = _positions(B, Nq, Nk, groups, kernel == "rope_cross", DEV)
    outs = []
    for _ in range(2):
        O = _new_out(groups, B * Nq, H * D, DEV)
        _launch(kernel, inputs, O, B, Nq, Nk, H, H * D, pos=pos)
        outs.append(O.view(torch.int16))
    assert torch.equal(outs[0], outs[1])


@gpu
def test_host_checks():
    """Bad arguments return S3_ERR_INVALID and launch nothing; Nq = 0 is OK and
    a no-op."""
    from splatt3r_amd import ops, _lib
    L = _lib.lib()
    B, Nq, Nk, H = 1, 16, 16, 1
    (q, k, v), = R.make_inputs("random", B, Nq, Nk, H, 1, seed=16, device=DEV)
    O = _new_out(1, Nq, D, DEV)
    cos, sin = _tables(DEV)
    qpos, kpos = _positions(B, Nq, Nk, 1, False, DEV)

    def args(**kw):
        a = ops.AttnArgs()
        a.B, a.Nq, a.Nk, a.H, a.groups = B, Nq, Nk, H, 1
        for g in range(4):      # five groups would read a fifth pointer: all four are valid
            a.Q[g], a.K[g], a.V[g], a.O[g] = q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr()
        a.q_stride = a.k_stride = a.v_stride = a.o_stride = D
        a.scale = SCALE
        for name, val in kw.items():
            if isinstance(val, tuple):
                getattr(a, name)[val[0]] = val[1]
            else:
                setattr(a, name, val)
        return a

    INVALID, OK = 1, 0          # S3_ERR_INVALID, S3_OK (include/s3_common.h)
    bad = {"Nk = 0": args(Nk=0), "B = 0": args(B=0), "groups = 5": args(groups=5),
           "groups = 0": args(groups=0), "H = 0": args(H=0), "Nq < 0": args(Nq=-1),
           "q_stride % 8": args(q_stride=D + 4), "k_stride % 8": args(k_stride=D + 4),
           "v_stride % 8": args(v_stride=D + 1),
           "null Q": args(Q=(0, None)), "null K": args(K=(0, None)), "null V": args(V=(0, None)),
           "null O": args(O=(0, None)),
           "null K of group 2": args(groups=2, K=(1, None)),
           "qpos without tables": args(qpos=(0, qpos[0].data_ptr())),
           "kpos without tables": args(kpos=(0, kpos[0].data_ptr())),
           "positions with cos only": args(qpos=(0, qpos[0].data_ptr()), rope_cos=cos.data_ptr())}
    for what, a in bad.items():
        assert L.s3n_attention(ctypes.byref(a), _lib.stream()) == INVALID, what
        assert L.s3_last_error(), what
    a = args(Nq=0)
    assert L.s3n_attention(ctypes.byref(a), _lib.stream()) == OK
    torch.cuda.synchronize()
    assert bool((O.view(torch.int16) == SENTINEL).all()), "a rejected call or Nq = 0 wrote to O"
    # the same struct with nothing wrong runs
    a = args()
    assert L.s3n_attention(ctypes.byref(a), _lib.stream()) == OK
    torch.cuda.synchronize()
    assert not bool((O.view(torch.int16) == SENTINEL).any())


@gpu
def test_headroom_report(parity):
    """Worst err / tol per kernel and family of test_kernels_vs_ref64 (uniform
    included), into the parity report."""
    if not HEADROOM:          # run on its own: nothing to report
        return
    for (kernel, family, tiles), ratio in sorted(HEADROOM.items()):
        parity(f"{kernel}/{family}/{tiles}", err=ratio, tol=1.0)
    assert max(HEADROOM.values()) <= 1.0
