"""The GEMM tile table (csrc/net_gemm_tiles.def, read through
s3n_gemm_tile_info): the CPU tests check the table and the views ops.py
builds from it; the GPU tests launch every tile the table lists and check
that the reduction classes ops.reduction_class derives from the table are
what the kernels compute (bit-identical outputs within a class)."""
import collections
import ctypes

import pytest
import torch
import torch.nn.functional as F

from splatt3r_amd import _lib, ops


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _rand(*shape, scale=1.0, dtype=torch.float16, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


# ---- CPU: the table and its views ------------------------------------------

def test_table_enumerates_with_unique_ids():
    L = _lib.lib()
    n = L.s3n_gemm_tile_count()
    ids = []
    for i in range(n):
        t = ops.GemmTile()
        assert L.s3n_gemm_tile_info(i, ctypes.byref(t)) == 0
        ids.append(t.id)
        assert t.id > 0 and t.bm > 0 and t.bn > 0 and t.bk in (64, 128) and t.kg >= 1
        assert t.mf in (16, 32)
    assert n > 0 and len(set(ids)) == n
    assert set(ids) == set(ops.tile_table().all)


@pytest.mark.parametrize("index", [-1, None])
def test_tile_info_rejects_an_out_of_range_index(index):
    L = _lib.lib()
    if index is None:
        index = L.s3n_gemm_tile_count()
    t = ops.GemmTile()
    assert L.s3n_gemm_tile_info(index, ctypes.byref(t)) == 1
    assert b"s3n_gemm_tile_info" in L.s3_last_error()


def test_views_are_consistent():
    t = ops.tile_table()
    assert t.shapes and set(t.red) == set(t.shapes)
    for view in (t.tail_ok, t.halo, t.bdirect, t.regs_epilogue):
        assert view <= set(t.shapes)
    assert list(t.shapes) == sorted(t.shapes)       # the tuner tries tiles in id order
    assert set(t.shapes) == {i for i, x in t.all.items() if x.tuner}
    assert not (t.halo & t.bdirect)


def test_mf16_tiles_never_take_the_register_epilogue():
    """launch<> / launch_pp<> static_assert that a 16x16x32 tile's fp32 image
    fits its LDS ring; the table's regs_epilogue must agree."""
    t = ops.tile_table()
    mf16 = [x for x in t.all.values() if x.mf == 16]
    assert mf16
    assert not [x.id for x in mf16 if x.regs_epilogue]
    assert not [i for i in t.regs_epilogue if t.red[i][2] == 16]


# ---- GPU: the table against the kernels ------------------------------------

# M ragged against every BM; N ragged against 64 / 96 / 128 / 160 / 192 / 256
# but a multiple of 8 (vector epilogue); K = 15.5 tiles of 64: a K tail, an
# uneven split over 2 and 3 K-groups, and K % 32 == 0 for the B-direct tiles
M, N, K, GROUPS = 130, 296, 992, 2


@pytest.fixture(scope="module")
def dense_case():
    A = [_rand(M, K, seed=g) for g in range(GROUPS)]
    W = [_rand(N, K, scale=K ** -0.5, seed=10 + g) for g in range(GROUPS)]
    b = [_rand(N, dtype=torch.float32, seed=20 + g) for g in range(GROUPS)]
    R = [_rand(M, N, dtype=torch.float32, seed=30 + g) for g in range(GROUPS)]
    ref = [F.gelu(A[g].float() @ W[g].float().T + b[g]) + R[g] for g in range(GROUPS)]
    return A, W, b, R, ref


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 2])
def test_dense_tiles_bitexact_within_their_reduction_class(dense_case, split):
    """Every tile that takes dense A -- the unoffered ones and the B-direct
    tiles (ops.gemm packs B for them) included -- with bias + GELU + fp32
    residual and fp16 output: bit-identical within ops.reduction_class, one
    member of each class against torch (test_net_ops.py's GEMM tolerance)."""
    A, W, b, R, ref = dense_case
    table = ops.tile_table().all
    dense = sorted(i for i, t in table.items() if not t.halo)
    assert {7, 60, 62, 64, 66} <= set(dense) and any(table[i].bdirect for i in dense)
    classes = collections.defaultdict(list)
    for tile in dense:
        C = [torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16)
             for _ in range(GROUPS)]
        ops.gemm(A, W, C, M, N, K, lda=K, bias=b, act="gelu", R1=R, ldr1=N, split_k=split,
                 tile=tile)(_lib.stream())
        classes[ops.reduction_class(K, tile, split)].append((tile, C))
    assert len(classes) > 1
    for cls, members in classes.items():
        t0, C0 = members[0]
        for g in range(GROUPS):
            err = rel_err(C0[g], ref[g])
            assert err < 2e-3, (t0, g, err)
        for tile, C in members[1:]:
            for g in range(GROUPS):
                assert torch.equal(C[g], C0[g]), (cls, t0, tile, g)


@pytest.mark.gpu
def test_halo_tiles_bitexact_within_their_reduction_class():
    """One 3x3 stride-1 conv, W = 256 (the smallest width BM = 128 and 256
    both divide); the 256x64 tiles get the first 64 output channels of the
    same weights, whose elements are the same sums."""
    B, H, Wd, Cin, Cout = 1, 3, 256, 64, 128
    x = _rand(B, H, Wd, Cin, seed=3)
    w = _rand(Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5, seed=4)
    bias = _rand(Cout, dtype=torch.float32, seed=5)
    wk = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), bias, padding=1).permute(0, 2, 3, 1)
    conv = dict(H=H, W=Wd, C=Cin, k=3, stride=1, pad=1, oH=H, oW=Wd)
    table = ops.tile_table().all
    halo = sorted(i for i, t in table.items() if t.halo)
    assert halo
    classes = collections.defaultdict(list)
    for tile in halo:
        co = 64 if table[tile].bn == 64 else Cout
        out = torch.full((B, H, Wd, co), float("nan"), device="cuda")
        ops.gemm([x], [wk[:co].contiguous()], [out], B * H * Wd, co, 9 * Cin, lda=0,
                 bias=[bias[:co].contiguous()], conv=conv, split_k=1, tile=tile)(_lib.stream())
        classes[ops.reduction_class(9 * Cin, tile, 1)].append((tile, out))
    for cls, members in classes.items():
        t0, out0 = members[0]
        err = rel_err(out0, ref[..., :out0.shape[-1]])
        assert err < 1e-5, (t0, err)
        for tile, out in members[1:]:
            co = min(out.shape[-1], out0.shape[-1])
            assert torch.equal(out[..., :co], out0[..., :co]), (cls, t0, tile)


@pytest.mark.gpu
def test_a_tile_the_table_does_not_list_is_an_error():
    assert 999 not in ops.tile_table().all
    A, W = [_rand(64, 64)], [_rand(64, 64, seed=1)]
    C = [torch.empty(64, 64, device="cuda")]
    with pytest.raises(RuntimeError, match="unknown tile"):
        ops.gemm(A, W, C, 64, 64, 64, lda=64, split_k=1, tile=999)(_lib.stream())
