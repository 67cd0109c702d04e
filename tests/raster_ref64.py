"""Dense differentiable float64 restatement of the splat rasterizer's forward
(include/gsr.h, DESIGN.md "Rasterizer"), for tests/test_raster_grad.py.

Plain PyTorch on the CPU.  No tile lists and no sorting network: every
Gaussian is evaluated against every pixel in view-depth order and the
transmittance is an exclusive cumulative product along the sorted axis.  The
gradients come from autograd; no derivative formula of the HIP kernels or of
oracle/raster_ref.c is restated here, so a transcription error shared by
those two shows up as a disagreement with this file.

Discrete rules (masks computed under torch.no_grad(); they carry no
gradient): view z <= 0.2 cull, det == 0 cull, radius
ceil(3 sqrt(max(l1, l2))) with the max(0.1, .) discriminant floor, the 16x16
tile rectangle (a Gaussian reaches only pixels whose tile lies inside it), the
power > 0 skip, the alpha < 1/255 skip, the test_T < 1e-4 stop (nothing later
contributes to that pixel), the SH colour clamp max(sum + 0.5, 0).

Conventions: the three places where the canonical backward is NOT the true
derivative of the forward.  Kernel and oracle both restate them; here each is
one explicit detach:
  1. Jacobian clamp: where |tx/tz| (|ty/tz|) exceeds 1.3 tan(fov), the
     clamped tx = lim * tz enters J as a constant: (lim * tz).detach().
  2. alpha = min(0.99, o G) is straight-through: the clamp changes the value,
     not the gradient.
  3. Depth order, radius and tile rectangle carry no gradient.
Two further constants of the canonical code are part of the forward and so
of this file: 1 / (w + 1e-7) in the perspective divide.  The canonical conic
backward divides by det^2 + 1e-7 where the true derivative has det^2; with
det >= 0.09 (the 0.3 low-pass) that is a relative 1.2e-5 at worst and below
1e-6 for the scenes of the test, i.e. part of the measured floor.

`ablate` removes one term from the graph (same forward value, different
gradient), for the sensitivity tests:
  "viewdir"    the SH view direction is detached
  "bg"         the T * bg term is detached
  "vm_T"       the gradient flows through the transposed rotation block of
               the view matrix
  "scale_mod"  the gradient of scale_modifier * scales is that of scales
"""
import numpy as np
import torch

BX = BY = 16
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005,
         -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
         -0.4570457994644658, 1.445305721320277, -0.5900435899266435)

GRAD_NAMES = ("dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
              "dL_dscales", "dL_drotations")


def sh_basis(deg, d):
    """Real SH basis (graphdeco sign convention), d [P, 3] unit -> [P, (deg+1)^2]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    B = [torch.full_like(x, SH_C0)]
    if deg > 0:
        B += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz,
              SH_C2[4] * (xx - yy)]
    if deg > 2:
        B += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
              SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy),
              SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)]
    return torch.stack(B, -1)


def _st(true, alt):
    """Value of `true`, gradient of `alt`."""
    return alt + (true - alt).detach()


def _near_int(v, eps):
    return (v - torch.round(v)).abs() < eps


def render(settings, means3D, opacities, shs=None, colors_precomp=None, scales=None,
           rotations=None, cov3D_precomp=None, dL_dout=None, dtype=torch.float64, ablate=()):
    """Same inputs as oracle.raster.  Returns a dict: color [3,H,W], radii [P]
    (numpy); with dL_dout the gradients under the oracle's names (numpy,
    float64), dL_dcolors / dL_dcov3D being those of the colour / covariance
    the blend / projection consumed whether leaf or not; and, from the values
    of this run alone: fragile_px [H,W], fragile_g [P], visible [P],
    sh_clamped [P,3], jclamp [P] (bool numpy), alpha_clamped (number of
    blended (Gaussian, pixel) pairs with o G > 0.99)."""
    dt = dtype
    grad = dL_dout is not None

    def leaf(a, shape):
        if a is None:
            return None
        t = torch.as_tensor(np.asarray(a, np.float64), dtype=dt).reshape(shape).clone()
        return t.requires_grad_(grad)

    cst = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dt)
    H, W = int(settings["image_height"]), int(settings["image_width"])
    gx, gy = (W + BX - 1) // BX, (H + BY - 1) // BY
    tanx, tany = float(settings["tanfovx"]), float(settings["tanfovy"])
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    mod = float(settings.get("scale_modifier", 1.0))
    D = int(settings["sh_degree"])
    bg = cst(settings["bg"]).reshape(3)
    vm = cst(settings["viewmatrix"]).reshape(4, 4)   # row-vector convention: p_view = [p 1] vm
    pm = cst(settings["projmatrix"]).reshape(4, 4)
    campos = cst(settings["campos"]).reshape(3)
    Rw, tw = vm[:3, :3].T, vm[3, :3]                 # p_view = Rw p + tw

    m = leaf(means3D, (-1, 3))
    P = m.shape[0]
    m2 = torch.zeros(P, 3, dtype=dt, requires_grad=grad)
    op = leaf(opacities, (P,))
    sh = leaf(shs, (P, -1, 3))
    col = leaf(colors_precomp, (P, 3))
    sc, rot = leaf(scales, (P, 3)), leaf(rotations, (P, 4))
    cov_in = leaf(cov3D_precomp, (P, 6))

    # ---- cull at the near plane; culled rows run on a harmless stand-in point
    with torch.no_grad():
        z0 = m @ Rw[2] + tw[2]
        valid_z = z0 > 0.2
        front = torch.linalg.solve(Rw, torch.tensor([0.0, 0.0, 3.0], dtype=dt) - tw)
    ms = torch.where(valid_z[:, None], m, front[None])

    def through_R(f):
        return _st(f(Rw), f(Rw.T)) if "vm_T" in ablate else f(Rw)

    t = through_R(lambda R: ms @ R.T) + tw
    tz = t[:, 2]
    limx, limy = 1.3 * tanx, 1.3 * tany
    rx, ry = t[:, 0] / tz, t[:, 1] / tz
    with torch.no_grad():
        inx = ~((rx < -limx) | (rx > limx))
        iny = ~((ry < -limy) | (ry > limy))
    txc = torch.where(inx, t[:, 0], (rx.clamp(-limx, limx) * tz).detach())   # convention 1
    tyc = torch.where(iny, t[:, 1], (ry.clamp(-limy, limy) * tz).detach())
    J00, J02 = fx / tz, -(fx * txc) / (tz * tz)
    J11, J12 = fy / tz, -(fy * tyc) / (tz * tz)
    T0 = through_R(lambda R: J00[:, None] * R[0][None] + J02[:, None] * R[2][None])
    T1 = through_R(lambda R: J11[:, None] * R[1][None] + J12[:, None] * R[2][None])

    # ---- 3-D covariance
    if cov_in is not None:
        cov6 = cov_in
    else:
        r, x, y, z = rot[:, 0], rot[:, 1], rot[:, 2], rot[:, 3]   # raw, not normalised
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)],
                        -1).reshape(P, 3, 3)
        s = mod * sc
        if "scale_mod" in ablate:
            s = _st(s, sc)
        Mm = R * s[:, None, :]
        S = Mm @ Mm.transpose(1, 2)
        cov6 = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2],
                            S[:, 2, 2]], -1)
        if grad:
            cov6.retain_grad()
    V = torch.stack([cov6[:, 0], cov6[:, 1], cov6[:, 2], cov6[:, 1], cov6[:, 3], cov6[:, 4],
                     cov6[:, 2], cov6[:, 4], cov6[:, 5]], -1).reshape(P, 3, 3)
    TV0 = torch.einsum("pi,pij->pj", T0, V)
    TV1 = torch.einsum("pi,pij->pj", T1, V)
    a = (TV0 * T0).sum(-1) + 0.3
    b = (TV0 * T1).sum(-1)
    c = (TV1 * T1).sum(-1) + 0.3
    det = a * c - b * b
    with torch.no_grad():
        det_ok = det != 0
        mid = 0.5 * (a + c)
        disc = torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        r3 = 3.0 * torch.sqrt(torch.maximum(mid + disc, mid - disc))
        rad = torch.ceil(r3)
    dets = torch.where(det_ok, det, torch.ones_like(det))
    cA, cB, cC = c / dets, -b / dets, a / dets

    # ---- screen position (means2D: an NDC offset, zero)
    ph = ms @ pm[:3] + pm[3]
    pw = 1.0 / (ph[:, 3] + 0.0000001)
    px = ((ph[:, 0] * pw + m2[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((ph[:, 1] * pw + m2[:, 1] + 1.0) * H - 1.0) * 0.5
    with torch.no_grad():
        ex = [(px - rad) / BX, (px + rad + BX - 1) / BX, (py - rad) / BY, (py + rad + BY - 1) / BY]
        x0 = torch.trunc(ex[0]).clamp(0, gx)
        x1 = torch.trunc(ex[1]).clamp(0, gx)
        y0 = torch.trunc(ex[2]).clamp(0, gy)
        y1 = torch.trunc(ex[3]).clamp(0, gy)
        visible = valid_z & det_ok & ((x1 - x0) * (y1 - y0) > 0)

    # ---- colour
    sh_sum = None
    if col is not None:
        rgb = col * 1.0
    else:
        o = ms - campos
        d = o / o.norm(dim=-1, keepdim=True)
        if "viewdir" in ablate:
            d = d.detach()
        nb = (D + 1) * (D + 1)
        sh_sum = torch.einsum("pk,pkc->pc", sh_basis(D, d), sh[:, :nb]) + 0.5
        rgb = torch.clamp(sh_sum, min=0.0)
    if grad:
        rgb.retain_grad()

    # ---- dense blend in depth order (stable: ties by Gaussian index)
    with torch.no_grad():
        key = torch.where(visible, tz, torch.full_like(tz, float("inf")))
        order = torch.sort(key, stable=True).indices
        xs = torch.arange(W, dtype=dt)
        ys = torch.arange(H, dtype=dt)
        tix, tiy = torch.div(xs, BX, rounding_mode="floor"), torch.div(ys, BY, rounding_mode="floor")
        inx_t = (tix[None] >= x0[order, None]) & (tix[None] < x1[order, None])   # [P, W]
        iny_t = (tiy[None] >= y0[order, None]) & (tiy[None] < y1[order, None])   # [P, H]
        inrect = visible[order, None, None] & iny_t[:, :, None] & inx_t[:, None, :]
    sel = lambda v: v[order][:, None, None]
    dx = sel(px) - xs[None, None, :]
    dy = sel(py) - ys[None, :, None]
    power = -0.5 * (sel(cA) * dx * dx + sel(cC) * dy * dy) - sel(cB) * dx * dy
    with torch.no_grad():
        cand = inrect & ~(power > 0)
    G = torch.exp(torch.where(cand, power, torch.zeros_like(power)))
    a_raw = sel(op) * G
    alpha = a_raw + (a_raw.clamp(max=0.99) - a_raw).detach()              # convention 2
    with torch.no_grad():
        act = cand & ~(alpha < 1.0 / 255.0)
        w0 = torch.where(act, alpha, torch.zeros_like(alpha))
        Tin0 = torch.cumprod(1.0 - w0, 0)
        Tex0 = torch.cat([torch.ones_like(Tin0[:1]), Tin0[:-1]], 0)
        test_T = Tex0 * (1.0 - alpha)
        stop = act & (test_T < 0.0001)
        done_incl = torch.cumsum(stop.to(torch.int32), 0) > 0
        done_before = done_incl & ~(stop & (torch.cumsum(stop.to(torch.int32), 0) == 1))
        contrib = act & ~done_incl
    w = torch.where(contrib, alpha, torch.zeros_like(alpha))
    Tin = torch.cumprod(1.0 - w, 0)
    Tex = torch.cat([torch.ones_like(Tin[:1]), Tin[:-1]], 0)
    C = torch.einsum("pc,phw->chw", rgb[order], w * Tex)
    Tfin = Tin[-1] if P > 0 else torch.ones(H, W, dtype=dt)
    out = C + (Tfin.detach() if "bg" in ablate else Tfin) * bg[:, None, None]

    res = dict(color=out.detach().numpy().astype(np.float64),
               radii=(rad * visible).to(torch.int32).numpy(),
               visible=visible.numpy(),
               jclamp=(visible & ~(inx & iny)).numpy(),
               sh_clamped=(None if sh_sum is None else (sh_sum.detach() < 0).numpy()),
               alpha_clamped=int((contrib & (a_raw.detach() > 0.99)).sum()))

    # ---- fragility: where a discrete rule sits close enough to its threshold
    # that float32 rounding may decide it the other way
    with torch.no_grad():
        live = cand & ~done_before
        fr_a = live & ((alpha - 1.0 / 255.0).abs() <= 1e-3 / 255.0)
        fr_t = act & ~done_before & ((test_T - 0.0001).abs() <= 1e-3 * 0.0001)
        res["fragile_px"] = (fr_a | fr_t).any(0).numpy()
        fg = (z0 - 0.2).abs() < 1e-4
        vis_math = valid_z & det_ok
        f2 = _near_int(r3, 1e-3)
        for e in ex:
            f2 = f2 | _near_int(e, 1e-3)
        f2 = f2 | ((rx.abs() / limx - 1.0).abs() < 1e-4) | ((ry.abs() / limy - 1.0).abs() < 1e-4)
        if sh_sum is not None:
            f2 = f2 | (sh_sum.abs() < 1e-4).any(-1)
        fg = fg | (vis_math & f2)
        ov = (x0[:, None] < x1[None]) & (x0[None] < x1[:, None]) & \
             (y0[:, None] < y1[None]) & (y0[None] < y1[:, None]) & \
             visible[:, None] & visible[None] & ~torch.eye(P, dtype=torch.bool)
        tie = ov & ((tz[:, None] - tz[None]).abs() < 1e-5 * tz[:, None])
        res["fragile_g"] = (fg | tie.any(1)).numpy()

    if grad:
        g = cst(dL_dout).reshape(3, H, W)
        (out * g).sum().backward()
        zero = lambda t_: torch.zeros_like(t_) if t_.grad is None else t_.grad
        res["dL_dmeans2D"] = zero(m2).numpy().astype(np.float64)
        res["dL_dopacity"] = zero(op).numpy().astype(np.float64)
        res["dL_dcolors"] = zero(rgb).numpy().astype(np.float64)
        res["dL_dmeans3D"] = zero(m).numpy().astype(np.float64)
        res["dL_dcov3D"] = zero(cov6).numpy().astype(np.float64)
        if sh is not None:
            res["dL_dsh"] = zero(sh).numpy().astype(np.float64)
        if sc is not None:
            res["dL_dscales"] = zero(sc).numpy().astype(np.float64)
            res["dL_drotations"] = zero(rot).numpy().astype(np.float64)
    return res
