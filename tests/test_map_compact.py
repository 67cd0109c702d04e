"""Map compaction (include/s3v.h, csrc/map_compact.hip, splatt3r_amd.compact):
the numpy float64 reference on hand-worked cases (CPU), then the HIP pass
against it, its determinism and idempotence, and SharedGaussians' use of it in
place of the eviction."""
import numpy as np
import pytest

import map_compact_ref64 as R

TOL = 2.0 ** -23     # float32's half-ulp rounding of a double-accurate value, doubled
                     # for the freedom in summation order


# ------------------------------------------------------------------ CPU ----
def test_ref_two_gaussian_group_by_hand():
    # voxel 1, origin 0: both centres in cell (0, 0, 0); every number dyadic
    means = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]], np.float32)
    cov = np.array([[0.5, 0, 0, 0.25, 0, 0.125], [0.25, 0, 0, 0.25, 0, 0.5]], np.float32)
    col = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    op = np.array([0.25, 0.75], np.float32)
    r = R.merge_ref(means, cov, col, op, np.array([3, 9], np.int32), 1.0)
    assert r["m"] == 1 and r["dropped"] == 0
    # W = 1; mu_x = 0.25 * 0.25 + 0.75 * 0.75 = 0.625, offsets -0.375 and 0.125
    assert r["means"].tolist() == [[0.625, 0.5, 0.5]]
    # xx = 0.25 (0.5 + 0.140625) + 0.75 (0.25 + 0.015625) = 0.359375
    # yy = 0.25; zz = 0.25 * 0.125 + 0.75 * 0.5 = 0.40625
    assert r["cov_triu"].tolist() == [[0.359375, 0, 0, 0.25, 0, 0.40625]]
    assert r["colors"].tolist() == [[0.25, 0.75, 0.0]]
    assert r["opacities"].tolist() == [0.625]          # 0.25^2 + 0.75^2, not stacked
    assert r["kf_id"].tolist() == [3] and r["first"].tolist() == [0]
    assert r["group"].tolist() == [0, 0] and r["size"].tolist() == [2]


def test_ref_keys_on_a_boundary_and_negative():
    b = R.BIAS
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    x = np.array([[1.0, -0.25, -0.5], [below, 0.0, -0.5000001]], np.float32)
    c = R.voxel_cells(x, 0.5)
    assert c.tolist() == [[b + 2, b - 1, b - 1], [b + 1, b, b - 2]]
    k = R.voxel_keys(x, 0.5)
    assert int(k[0]) == ((b + 2) << 42) | ((b - 1) << 21) | (b - 1)
    # a shifted, non-integer origin; and the documented clamp
    assert R.voxel_cells(np.array([[0.0, -1.5, 3.0]], np.float32), 0.5,
                         (-1.25, -1.5, 3.25)).tolist() == [[b + 2, b, b - 1]]
    assert R.voxel_cells(np.array([[1e9, -1e9, 0.0]], np.float32), 0.01).tolist() == [[R.TOP, 0, b]]


def test_ref_all_zero_weights_fall_back_to_equal_weights():
    means = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [5.5, 0, 0]], np.float32)
    cov = np.zeros((3, 6), np.float32)
    col = np.array([[1, 0, 0], [0, 0, 1], [0.5, 0.5, 0.5]], np.float32)
    op = np.array([0.0, 0.0, 0.5], np.float32)
    r = R.merge_ref(means, cov, col, op, np.zeros(3, np.int32), 1.0)
    assert r["m"] == 2 and r["group"].tolist() == [0, 0, 1]
    assert r["means"][0].tolist() == [0.5, 0.25, 0.25]
    assert r["cov_triu"][0].tolist() == [0.0625, 0, 0, 0, 0, 0]
    assert r["colors"][0].tolist() == [0.5, 0, 0.5] and r["opacities"][0] == 0.0
    assert r["opacities"][1] == 0.5


def test_ref_drops_a_nan_row():
    means = np.array([[0.25, 0.25, 0.25], [np.nan, 0.25, 0.25], [0.75, 0.25, 0.25]], np.float32)
    cov = np.zeros((3, 6), np.float32)
    col = np.full((3, 3), 0.5, np.float32)
    op = np.array([0.5, 0.5, 0.5], np.float32)
    r = R.merge_ref(means, cov, col, op, np.array([4, 5, 6], np.int32), 1.0)
    assert r["m"] == 1 and r["dropped"] == 1
    assert r["group"].tolist() == [0, -1, 0]
    assert r["means"][0].tolist() == [0.5, 0.25, 0.25] and r["kf_id"].tolist() == [4]
    assert r["size"].tolist() == [2]


# ------------------------------------------------------------------ GPU ----
VOXEL = 0.05
ORIGINS = ((0.0, 0.0, 0.0), (-1.37, 2.21, -0.53))
# Besides the sizes the issue names: 2,049 is the first size at which a sort
# pass and the scans take a second workgroup (2,048 rows each; the chunked
# sums take one per 256 rows, so 257 already has two), and 2,097,153 the first
# at which the top scan over those workgroups' sums (1,024 per trip) takes a
# second trip; its group of 20,000 rows is past the 16,384 at which a thread of
# the long-group pass takes a second chunk.  2,047 and 2,048 are one row short
# of a sort segment and exactly one segment.
SIZES = (1, 2, 257, 2047, 2048, 2049, 4099, 2097153)


def _sizes_of_groups(n, rng):
    """Group sizes summing to n: one of 20,000 (n permitting), one of 3,000
    (longer than a workgroup), some of about 40, pairs and singles."""
    sizes = []
    left = n
    for big, least in ((20000, 1 << 20), (3000, 4099)):
        if n >= least:
            sizes.append(big)
            left -= big
    for _ in range(3 if n > 200 else 0):
        sizes.append(int(rng.integers(36, 45)))
        left -= sizes[-1]
    small = rng.choice([1, 1, 2, 2, 3, 5], size=max(left, 0))
    upto = np.cumsum(small)
    k = int(np.searchsorted(upto, left))          # the first k + 1 reach `left`
    if left > 0:
        small = small[:k + 1]
        small[k] -= upto[k] - left
        sizes += small.tolist()
    if n == 2:
        sizes = [2]
    return np.array(sizes, np.int64)


def make_map(n, seed, origin, voxel=VOXEL):
    """n Gaussians in random row order whose groups have the sizes above, with
    a few centres exactly on a voxel face."""
    rng = np.random.default_rng(seed)
    sizes = _sizes_of_groups(n, rng)
    G = len(sizes)
    side = 200
    ids = rng.choice(side ** 3, size=G, replace=False)
    cells = np.stack([ids // side ** 2, ids // side % side, ids % side], 1) - side // 2
    gid = np.repeat(np.arange(G), sizes)
    u = rng.uniform(0.05, 0.95, (n, 3))
    # members of small groups exactly on a voxel face: whichever side float32
    # puts them on, the kernel and the reference must agree
    on_face = (rng.random(n) < 0.05) & (sizes[gid] <= 5)
    u[on_face, 0] = 0.0
    means = (np.asarray(origin) + (cells[gid] + u) * voxel).astype(np.float32)
    # diagonally dominant, so positive definite: xx xy xz yy yz zz
    cov = rng.uniform(-0.3, 0.3, (n, 6))
    cov[:, [0, 3, 5]] = rng.uniform(1.0, 2.0, (n, 3))
    cov = (cov * (0.1 * voxel) ** 2).astype(np.float32)
    col = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    op = rng.uniform(0.05, 1, n).astype(np.float32)
    perm = rng.permutation(n)
    kf = np.sort(rng.integers(0, 9, n)).astype(np.int32)
    return means[perm], cov[perm], col[perm], op[perm], kf


def _dev(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _host(outs):
    return [t.cpu().numpy() for t in outs]


def _check_against_ref(got, ref, inputs, label, parity=None):
    means, cov, col, op, kf, first, group, m, dropped = got
    m, dropped = int(m), int(dropped)
    assert m == ref["m"] and dropped == ref["dropped"], label
    n = len(ref["group"])
    assert np.array_equal(first[:m], ref["first"]), label
    assert np.array_equal(group[:n], ref["group"]), label
    assert np.array_equal(kf[:m], ref["kf_id"]), label
    for name, g, w in (("means", means, 3), ("cov_triu", cov, 6), ("colors", col, 3),
                       ("opacities", op, 1)):
        want = ref[name].reshape(m, w)
        have = g[:m].astype(np.float64).reshape(m, w)
        bound = TOL * np.abs(want).max(1, keepdims=True)
        worst = float((np.abs(have - want) / np.maximum(bound, 1e-300)).max()) if m else 0.0
        print(f"{label} {name}: worst error / bound = {worst:.3f}")
        if parity is not None:
            parity(f"map_compact.{label}.{name}", err=worst, tol=1.0)
        assert (np.abs(have - want) <= bound).all(), (label, name, worst)
    # a group of one is its input, bit for bit
    one = np.flatnonzero(ref["size"] == 1)
    src = ref["first"][one]
    for g, x in zip((means, cov, col, op), inputs[:4]):
        assert np.array_equal(g[:m][one].view(np.uint32), x[src].view(np.uint32)), label
    # every merged covariance is positive semi-definite up to rounding
    c = cov[:m].astype(np.float64)
    full = c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(m, 3, 3)
    low = np.linalg.eigvalsh(full)[:, 0] if m else np.zeros(0)
    assert (low >= -TOL * np.abs(c).max(1)).all(), label


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_hip_merge_matches_ref(n, parity):
    import torch
    from splatt3r_amd.compact import merge_gaussians
    large = n > 100000
    for k, origin in enumerate(ORIGINS):
        if large and k == 0:
            # the large size once, at the awkward origin and with n_dev < n_max
            # only: a full-length run and the other origin would each add the
            # reference's and the input's 3 s and reach no code the run below
            # does not (the second trip of the top scan and of the long-group
            # pass both depend on n_max and on the 20,000-row group alone)
            continue
        inputs = make_map(n, 100 + n % 97 + k, origin)
        dev = _dev(inputs)
        if not large:
            ref = R.merge_ref(*inputs, VOXEL, origin)
            if n >= 4099:
                assert {3000, 2, 1} <= set(ref["size"].tolist())
                assert ((ref["size"] > 30) & (ref["size"] < 50)).any()
            got = _host(merge_gaussians(*dev, VOXEL, origin))
            _check_against_ref(got, ref, inputs, f"n{n}.o{k}", parity)
        # a device count below the tensors' size: the rows past it do not exist
        # (the large size runs this way only; its 20,000-row group loses a
        # seventh of its rows and stays past 16,384)
        live = n - n // 7 if n > 2 else n
        ref = R.merge_ref(*inputs, VOXEL, origin, n=live)
        cnt = torch.tensor([live], dtype=torch.int64, device="cuda")
        got = _host(merge_gaussians(*dev, VOXEL, origin, n=cnt))
        assert (got[6][live:] == -1).all()
        if large:
            assert ref["size"].max() > 16384 and (ref["size"] > 2048).sum() == 2
        _check_against_ref(got, ref, inputs, f"n{n}.o{k}.live{live}", parity if large else None)


@pytest.mark.gpu
def test_hip_merge_is_deterministic_and_idempotent():
    import torch
    from splatt3r_amd.compact import merge_gaussians
    origin = ORIGINS[1]
    dev = _dev(make_map(4099, 7, origin))
    a = merge_gaussians(*dev, VOXEL, origin)
    b = merge_gaussians(*dev, VOXEL, origin)
    m = int(a[7])
    assert 0 < m < 4099 and int(b[7]) == m and int(a[8]) == int(b[8]) == 0
    for x, y in zip(a[:6], b[:6]):          # rows at and past m are not written
        assert torch.equal(x[:m].view(x.dtype if x.dtype != torch.float32 else torch.int32),
                           y[:m].view(y.dtype if y.dtype != torch.float32 else torch.int32))
    assert torch.equal(a[6], b[6])
    again = merge_gaussians(*[t[:m].contiguous() for t in a[:5]], VOXEL, origin)
    assert int(again[7]) == m and int(again[8]) == 0
    for x, y in zip(a[:5], again[:5]):
        assert torch.equal(x[:m].view(torch.int32), y[:m].view(torch.int32))
    assert torch.equal(again[5][:m], torch.arange(m, device="cuda"))
    assert torch.equal(again[6][:m], torch.arange(m, device="cuda"))


@pytest.mark.gpu
def test_hip_merge_is_independent_of_row_order(parity):
    """Permuting the rows changes which row is `first` (and so the output
    order and the kf_id taken) and nothing else about a group beyond rounding:
    the same voxels with the same members, values within the parity bound of
    each other, `first` the lowest of the permuted indices."""
    from splatt3r_amd.compact import merge_gaussians
    origin = ORIGINS[1]
    n = 4099
    a_in = list(make_map(n, 13, origin))
    a_in[4] = np.arange(n, dtype=np.int32) * 3 + 1        # a kf_id that names its row
    rng = np.random.default_rng(14)
    perm = rng.permutation(n)                              # row i of b is row perm[i] of a
    where = np.argsort(perm)                               # row j of a is row where[j] of b
    b_in = [x[perm] for x in a_in]
    sizes = R.merge_ref(*a_in, VOXEL, origin)["size"]
    assert {3000, 2, 1} <= set(sizes.tolist()) and ((sizes > 30) & (sizes < 50)).any()
    a = _host(merge_gaussians(*_dev(a_in), VOXEL, origin))
    b = _host(merge_gaussians(*_dev(b_in), VOXEL, origin))
    m = int(a[7])
    assert int(b[7]) == m and int(a[8]) == int(b[8]) == 0
    ka = R.voxel_keys(a[0][:m], VOXEL, origin)
    kb = R.voxel_keys(b[0][:m], VOXEL, origin)
    assert len(set(ka.tolist())) == m and set(ka.tolist()) == set(kb.tolist())
    ra, rb = np.argsort(ka), np.argsort(kb)                # output rows of a and b, voxel by voxel
    # the same rows in every voxel: a's row j and b's row where[j] share a voxel
    row_b_of_row_a = np.empty(m, np.int64)
    row_b_of_row_a[ra] = rb
    assert np.array_equal(row_b_of_row_a[a[6]], b[6][where])
    assert np.array_equal(np.bincount(a[6], minlength=m)[ra], np.bincount(b[6], minlength=m)[rb])
    for name, k, w in (("means", 0, 3), ("cov_triu", 1, 6), ("colors", 2, 3), ("opacities", 3, 1)):
        x = a[k][:m][ra].astype(np.float64).reshape(m, w)
        y = b[k][:m][rb].astype(np.float64).reshape(m, w)
        bound = TOL * np.maximum(np.abs(x), np.abs(y)).max(1, keepdims=True)
        worst = float((np.abs(x - y) / np.maximum(bound, 1e-300)).max())
        print(f"row order {name}: worst difference / bound = {worst:.3f}")
        parity(f"map_compact.row_order.{name}", err=worst, tol=1.0)
        assert (np.abs(x - y) <= bound).all(), (name, worst)
    # first is the lowest permuted index of the group, kf_id that row's
    low = np.full(m, n, np.int64)
    np.minimum.at(low, b[6], np.arange(n))
    assert np.array_equal(b[5][:m], low)
    assert np.array_equal(b[4][:m], b_in[4][low])
    assert np.array_equal(a[4][:m], a_in[4][a[5][:m]])
    assert (np.diff(b[5][:m]) > 0).all()                   # output ordered by first
    assert (a[5][:m][ra] != perm[b[5][:m][rb]]).any()      # and first did change somewhere


@pytest.mark.gpu
def test_hip_merge_one_voxel_and_all_dropped(parity):
    """The two ends of the packed sort keys: every row in one voxel (no sort
    pass at all, one group of 65 chunks) and no kept row."""
    from splatt3r_amd.compact import merge_gaussians
    inputs = make_map(4099, 9, ORIGINS[0])
    ref = R.merge_ref(*inputs, 1000.0, (-500.0, -500.0, -500.0))
    assert ref["m"] == 1 and ref["size"].tolist() == [4099]
    got = _host(merge_gaussians(*_dev(inputs), 1000.0, (-500.0, -500.0, -500.0)))
    _check_against_ref(got, ref, inputs, "one_voxel", parity)
    bad = [a.copy() for a in inputs]
    bad[3][:] = np.inf
    ref = R.merge_ref(*bad, VOXEL)
    assert ref["m"] == 0 and ref["dropped"] == 4099
    got = _host(merge_gaussians(*_dev(bad), VOXEL))
    _check_against_ref(got, ref, bad, "all_dropped")


@pytest.mark.gpu
def test_hip_merge_collapses_duplicates():
    import torch
    from splatt3r_amd.compact import merge_gaussians
    n = 1500
    rng = np.random.default_rng(5)
    ids = rng.choice(60 ** 3, size=n, replace=False)
    cells = np.stack([ids // 3600, ids // 60 % 60, ids % 60], 1) - 30
    means = ((cells + rng.uniform(0.1, 0.9, (n, 3))) * VOXEL).astype(np.float32)
    _, cov, col, op, _ = make_map(n, 6, ORIGINS[0])
    one = _dev((means, cov, col, op))
    three = [torch.cat([t, t, t]) for t in one]
    kf = torch.arange(3, device="cuda", dtype=torch.int32).repeat_interleave(n) + 4
    got = merge_gaussians(*three, kf, VOXEL)
    assert int(got[7]) == n and int(got[8]) == 0
    for k in (0, 2, 3):                                  # means, colours, opacities
        assert torch.equal(got[k][:n].view(torch.int32), one[k].view(torch.int32))
    c, want = got[1][:n].double(), one[1].double()
    assert bool(((c - want).abs() <= TOL * want.abs().amax(1, keepdim=True)).all())
    assert bool((got[4][:n] == 4).all())                 # the first copy's kf_id
    assert torch.equal(got[5][:n], torch.arange(n, device="cuda"))   # the set's order
    assert torch.equal(got[6], torch.arange(n, device="cuda").repeat(3))


@pytest.mark.gpu
def test_hip_merge_bad_input(monkeypatch):
    import torch
    from splatt3r_amd import _lib, compact
    from splatt3r_amd.compact import merge_gaussians
    inputs = make_map(257, 11, ORIGINS[0])
    dev = _dev(inputs)
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            merge_gaussians(*dev, voxel)
    for origin in ((0.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0), (0.0, 0.0)):
        with pytest.raises(ValueError):
            merge_gaussians(*dev, VOXEL, origin)
    with pytest.raises(ValueError):
        merge_gaussians(dev[0], dev[1][:-1], *dev[2:], VOXEL)
    with pytest.raises(ValueError):
        merge_gaussians(*dev[:4], dev[4].long(), VOXEL)
    with pytest.raises(ValueError):
        merge_gaussians(*dev[:3], dev[3][:, None], dev[4], VOXEL)
    # non-finite rows are dropped and counted, the rest is as without them
    bad = [a.copy() for a in inputs]
    bad[0][10, 1] = np.nan
    bad[1][20, 4] = np.inf
    bad[3][30] = np.nan
    ref = R.merge_ref(*bad, VOXEL)
    assert ref["dropped"] == 3 and (ref["group"][[10, 20, 30]] == -1).all()
    _check_against_ref(_host(merge_gaussians(*_dev(bad), VOXEL)), ref, bad, "bad")
    # n = 0: empties, and the library is not entered
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a: calls.append(a))
    out = merge_gaussians(*[t[:0] for t in dev], VOXEL)
    assert not calls
    assert [tuple(t.shape) for t in out[:7]] == [(0, 3), (0, 6), (0, 3), (0,), (0,), (0,), (0,)]
    assert int(out[7]) == 0 and int(out[8]) == 0
    assert compact.merge_gaussians is merge_gaussians


# ------------------------------------------------- SharedGaussians -------
MAP_VOXEL = 0.1
CAP, PER = 4096, 1024


def _region(z_cell, seed, jitter=0.0):
    """1,024 Gaussians, one per voxel of a 32 x 32 sheet at height z_cell, at
    the voxel's centre plus up to `jitter` voxels per axis; opacity 0.5."""
    import torch
    rng = np.random.default_rng(seed)
    ix, iy = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    cells = np.stack([ix.ravel(), iy.ravel(), np.full(PER, z_cell)], 1)
    means = ((cells + 0.5 + rng.uniform(-jitter, jitter, (PER, 3))) * MAP_VOXEL)
    cov = np.tile(np.array([1, 0, 0, 1, 0, 1], np.float64) * (0.2 * MAP_VOXEL) ** 2, (PER, 1))
    col = rng.uniform(0, 1, (PER, 3))
    t = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    return t(means), t(cov), t(col), torch.full((PER,), 0.5, device="cuda")


def _keys_of(gm, n):
    return R.voxel_keys(gm.means[:n].cpu().numpy(), MAP_VOXEL)


def _fill(gm, regions):
    for k, r in enumerate(regions):
        gm.append(*r, kf_idx=k)
    return gm


@pytest.mark.gpu
def test_hip_map_compacts_instead_of_evicting():
    from splatt3r_amd.gaussian_map import SharedGaussians
    A, C = _region(0, 1), _region(10, 2)
    Bs = [_region(5, 3 + k, jitter=0.25) for k in range(3)]
    regions = [A, *Bs, C]
    kA, kB, kC = (R.voxel_keys(r[0].cpu().numpy(), MAP_VOXEL) for r in (A, Bs[0], C))
    assert len(set(kA) | set(kB) | set(kC)) == 3 * PER
    for b in Bs[1:]:
        assert set(R.voxel_keys(b[0].cpu().numpy(), MAP_VOXEL)) == set(kB)
    # the contrast, existing behaviour: region A is evicted
    plain = _fill(SharedGaussians(max_gaussians=CAP, device="cuda"), regions)
    assert plain.n_gaussians == 3 * PER and plain.n_compactions == 0
    assert plain.kf_id[:3 * PER].cpu().tolist() == [2] * PER + [3] * PER + [4] * PER
    assert not set(_keys_of(plain, 3 * PER)) & set(kA)
    # with compaction the three B's merge and nothing is lost
    gm = _fill(SharedGaussians(max_gaussians=CAP, device="cuda", compact_voxel=MAP_VOXEL), regions)
    assert gm.n_gaussians == 3 * PER
    assert gm.n_compactions == 1
    keys = _keys_of(gm, 3 * PER)
    assert sorted(keys.tolist()) == sorted(kA.tolist() + kB.tolist() + kC.tolist())
    kf = gm.kf_id[:3 * PER].cpu().numpy()
    assert (np.diff(kf) >= 0).all() and kf.tolist() == [0] * PER + [1] * PER + [4] * PER
    assert bool((gm.opacities[:3 * PER] == 0.5).all())


@pytest.mark.gpu
def test_hip_map_that_cannot_shrink_falls_back_to_eviction():
    from splatt3r_amd.gaussian_map import SharedGaussians
    regions = [_region(3 * k, 20 + k) for k in range(7)]
    gm = SharedGaussians(max_gaussians=CAP, device="cuda", compact_voxel=MAP_VOXEL)
    plain = SharedGaussians(max_gaussians=CAP, device="cuda")
    for k, r in enumerate(regions):
        gm.append(*r, kf_idx=k)
        plain.append(*r, kf_idx=k)
        assert gm.n_compactions == (1 if k >= 4 else 0)      # one, not one per append
    n = plain.n_gaussians
    assert gm.n_gaussians == n
    # compaction found only singletons: the map is the evicting map, bit for bit
    import torch
    for f in ("means", "cov_triu", "colors", "opacities", "kf_id"):
        assert torch.equal(getattr(gm, f)[:n], getattr(plain, f)[:n])
    # that compaction left the buffer full, so the growth rule stays unmet for
    # this map; clear() starts over: the rebuilt map compacts again
    gm.clear()
    _fill(gm, [_region(0, 1), *[_region(5, 3 + k, jitter=0.25) for k in range(3)],
               _region(10, 2)])
    assert gm.n_compactions == 2 and gm.n_gaussians == 3 * PER
    assert gm.kf_id[:3 * PER].cpu().tolist() == [0] * PER + [1] * PER + [4] * PER


@pytest.mark.gpu
def test_hip_map_without_compact_voxel_is_untouched(monkeypatch):
    import torch
    from splatt3r_amd import compact
    from splatt3r_amd.gaussian_map import SharedGaussians
    regions = [_region(0, 1), *[_region(5, 3 + k, jitter=0.25) for k in range(3)], _region(10, 2)]
    merges = []
    real = compact.launch_merge
    monkeypatch.setattr(compact, "launch_merge", lambda *a: (merges.append(1), real(*a)))
    omitted = _fill(SharedGaussians(max_gaussians=CAP, device="cuda"), regions)
    none = _fill(SharedGaussians(max_gaussians=CAP, device="cuda", compact_voxel=None), regions)
    assert not merges and omitted.n_compactions == none.n_compactions == 0
    assert omitted.n_gaussians == none.n_gaussians == 3 * PER
    for f in ("means", "cov_triu", "colors", "opacities", "kf_id"):
        a, b = getattr(omitted, f), getattr(none, f)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_hip_map_compact_then_refine():
    import torch
    from test_refine import H, W, _map_of, _map_rows, _scene
    from splatt3r_amd.gaussian_map import SharedGaussians
    from splatt3r_amd.refine import render_splats
    _, T_WC, K = _scene()
    t, start, kf = _map_rows()
    images = render_splats(t, T_WC, K, H, W)
    gm = _map_of(start, torch.sort(kf).values)
    n = gm.n_gaussians
    extent = float((gm.means[:n].amax(0) - gm.means[:n].amin(0)).max())
    m = gm.compact(extent / 12)                  # coarse enough that most rows merge
    print(f"compact: {n} -> {m}")
    assert 0 < m < n and gm.n_gaussians == m and gm.n_compactions == 1
    for f in (gm.means, gm.cov_triu, gm.colors, gm.opacities):
        assert bool(torch.isfinite(f[:m]).all())
    assert bool((gm.kf_id[:m].diff() >= 0).all())
    rows = gm.to_splats(m)                       # the merged rows through the eigendecomposition
    assert bool(torch.isfinite(rows).all())
    hist = gm.refine(images, T_WC, K, 2)
    assert hist.shape == (2,) and bool(torch.isfinite(hist).all())
    assert gm.n_gaussians == m
    for f in (gm.means, gm.cov_triu, gm.colors, gm.opacities):
        assert bool(torch.isfinite(f[:m]).all())
    assert SharedGaussians(max_gaussians=16, device="cuda").compact(0.1) == 0
