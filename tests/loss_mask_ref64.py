"""Float64 PyTorch restatement of the co-visibility loss mask (include/s3c.h):
unproject every target pixel with its depth, project it into every context
view, test the frustum, sample the context depth bilinearly with zero padding
at (u - 0.5, v - 0.5) and compare depths as torch.isclose(atol=0.1) does.

Beyond the mask and its three conditions it returns, per (pixel, context
view), the quantities the decisions hang on and their margins

    m_fr = min(|u|, |u - W|, |v|, |v - H|)      pixels to the frustum's edge
    m_md = |z - s| - (0.1 + 1e-5 |s|)           depth units to the isclose edge

so a test can tell the pixels whose decision float32 rounding may flip (a
margin inside the ambiguity band) from the ones where it must agree.
`dtype=torch.float32` runs the same graph in float32.
"""
import torch

ATOL = 1e-1
RTOL = 1e-5
MIN_DEPTH = 1e-6
COND_FRUSTUM, COND_DEPTH, COND_MATCH = 1, 2, 4


def bilinear_zeros(img, ix, iy):
    """img [h, w] sampled at the pixel-index coordinates ix, iy (any shape);
    a tap outside the image contributes 0.  Non-finite coordinates give NaN."""
    h, w = img.shape
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    out = torch.zeros_like(ix)
    flat = img.reshape(-1)
    for dx, dy, wt in ((0, 0, (1 - wy1) * (1 - wx1)), (1, 0, (1 - wy1) * wx1),
                       (0, 1, wy1 * (1 - wx1)), (1, 1, wy1 * wx1)):
        tx, ty = x0 + dx, y0 + dy
        inside = (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
        lin = torch.where(inside, ty * w + tx, torch.zeros_like(tx)).to(torch.int64)
        val = torch.where(inside, flat[lin], torch.zeros_like(ix))
        out = out + val * wt
    return out


def loss_mask_ref(depth_1, K_1, c2w_1, depth_2, K_2, c2w_2, dtype=torch.float64):
    """depth_1 [b, v1, h, w], K_1 [b, v1, 3, 3], c2w_1 [b, v1, 4, 4] and the
    same for the v2 context views.  Returns a dict: mask, fr, nz, md
    ([b, v1, h, w] bool; fr and md already reduced over the context views),
    conditions (uint8 bits) and u, v, z, s, m_fr, m_md ([b, v1, v2, h, w])."""
    depth_1, K_1, c2w_1, depth_2, K_2, c2w_2 = (
        t.to(dtype) for t in (depth_1, K_1, c2w_1, depth_2, K_2, c2w_2))
    b, v1, h, w = depth_1.shape
    v2 = depth_2.shape[1]
    Kinv = torch.linalg.inv(K_1.double()).to(dtype)
    w2c = torch.linalg.inv(c2w_2.double()).to(dtype)

    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype),
                            indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)                   # [h, w, 3]
    # cam[b, i, y, x, r] = sum_c Kinv[b, i, r, c] pix[y, x, c], times the depth
    cam = (Kinv[:, :, None, None] * pix[None, None, :, :, None, :]).sum(-1) * depth_1[..., None]
    R1, t1 = c2w_1[:, :, :3, :3], c2w_1[:, :, :3, 3]
    world = (R1[:, :, None, None] * cam[..., None, :]).sum(-1) + t1[:, :, None, None]
    R2, t2 = w2c[:, :, :3, :3], w2c[:, :, :3, 3]
    # cp[b, i, j, y, x, r]
    cp = (R2[:, None, :, None, None] * world[:, :, None, :, :, None, :]).sum(-1) \
        + t2[:, None, :, None, None]
    z = cp[..., 2]
    n = cp / z[..., None]
    uv = (K_2[:, None, :, None, None, :2, :] * n[..., None, :]).sum(-1)
    u, v = uv[..., 0], uv[..., 1]
    fr = (u > 0) & (u < w) & (v > 0) & (v < h)

    s = torch.empty_like(z)
    for bb in range(b):
        for j in range(v2):
            s[bb, :, j] = bilinear_zeros(depth_2[bb, j], u[bb, :, j] - 0.5, v[bb, :, j] - 0.5)
    m_md = (z - s).abs() - (ATOL + RTOL * s.abs())
    md = (z == s) | (m_md <= 0)
    m_fr = torch.minimum(torch.minimum(u.abs(), (u - w).abs()),
                         torch.minimum(v.abs(), (v - h).abs()))

    fr_any, md_any, nz = fr.any(2), md.any(2), depth_1 > MIN_DEPTH
    cond = (fr_any.to(torch.uint8) * COND_FRUSTUM + nz.to(torch.uint8) * COND_DEPTH
            + md_any.to(torch.uint8) * COND_MATCH)
    return dict(mask=fr_any & nz & md_any, fr=fr_any, nz=nz, md=md_any, conditions=cond,
                u=u, v=v, z=z, s=s, m_fr=m_fr, m_md=m_md)


def ambiguous(ref, eps_px, eps_d):
    """[b, v1, h, w] bool: some context view's frustum or depth margin lies
    inside the band.  A NaN margin (a point at z = 0) is not ambiguous: every
    comparison with it is false in any precision."""
    return ((ref["m_fr"] < eps_px) | (ref["m_md"].abs() < eps_d)).any(2)
