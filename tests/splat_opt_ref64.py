"""Reference of the splat optimiser (include/s3o.h): torch autograd through
the activations, then torch.optim.Adam, on the CPU, in float64 (the reference)
or float32 (the rounding floor).  Shares no code with csrc/splat_opt_math.hpp.

Packed layouts, all [n, 14] with the five groups in the same columns:
  rows14       x y z | f_dc | logit | log scale | rot w x y z (raw)
  activations  means3D | shs | opacity | scales | rotations (unit)
  gradients    dmeans3D | dshs | dopacity | dscales | drotations
"""
import ctypes

import numpy as np
import torch

from splat_ref64 import tolerance  # noqa: F401  (4 x floor, one significant digit up)

GROUPS = ("means", "f_dc", "opacity", "scale", "rotation")
SL = dict(means=slice(0, 3), f_dc=slice(3, 6), opacity=slice(6, 7), scale=slice(7, 10),
          rotation=slice(10, 14))
LR = dict(means=1.6e-4, f_dc=2.5e-3, opacity=0.05, scale=5e-3, rotation=1e-3)
f32 = lambda x: ctypes.c_float(x).value
# the ABI carries the hyperparameters as float32: the reference gets the same values
BETAS = (f32(0.9), f32(0.999))
EPS = f32(1e-15)
LRS = {g: f32(v) for g, v in LR.items()}
STEPS = 3
ZERO_QUAT_ROW = 7


def make_inputs(n=1000, seed=2024, steps=STEPS):
    """(rows14 [n, 14], grads [steps, n, 14]) float32.  Gradient magnitudes
    log-uniform over 1e-8..1e2 with random signs and 5 % exact zeros, logits in
    +-12, log-scales in -9..1, raw quaternion norms log-uniform in 0.1..10, row
    ZERO_QUAT_ROW a zero quaternion."""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, 14))
    rows[:, 0:3] = rng.normal(size=(n, 3)) * 3.0
    rows[:, 3:6] = rng.normal(size=(n, 3))
    rows[:, 6] = rng.uniform(-12.0, 12.0, n)
    rows[:, 7:10] = rng.uniform(-9.0, 1.0, (n, 3))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rows[:, 10:14] = q * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (n, 1)))
    rows[6 % n, 6], rows[8 % n, 6] = 12.0, -12.0
    rows[ZERO_QUAT_ROW % n, 10:14] = 0.0
    mag = np.exp(rng.uniform(np.log(1e-8), np.log(1e2), (steps, n, 14)))
    g = mag * rng.choice([-1.0, 1.0], mag.shape)
    g[rng.random(mag.shape) < 0.05] = 0.0
    return rows.astype(np.float32), g.astype(np.float32)


def activate(parts, s, ablate=()):
    """Five leaf tensors (xyz, f_dc, logit, log scale, quat) -> the packed
    activations [n, 14], differentiable."""
    xyz, fdc, logit, lsc, q = parts
    nn = q.norm(dim=1, keepdim=True)
    live = nn > 0
    safe = torch.where(live, nn, torch.ones_like(nn))
    if "quat_jacobian" in ablate:
        safe = safe.detach()
    ident = torch.zeros_like(q)
    ident[:, 0] = 1.0
    qh = torch.where(live, q / safe, ident)
    return torch.cat([s * xyz, fdc, torch.sigmoid(logit), s * torch.exp(lsc), qh], 1)


def _split(rows, dtype):
    t = torch.as_tensor(np.asarray(rows), dtype=dtype)
    return [t[:, SL[g]].clone().requires_grad_(True) for g in GROUPS]


def activations(rows, s, dtype=torch.float64):
    with torch.no_grad():
        return activate(_split(rows, dtype), float(s)).numpy()


def run(rows, grads, s, dtype=torch.float64, ablate=(), manual=False, lrs=LRS, betas=BETAS,
        eps=EPS):
    """Consecutive steps with carried state.  Returns a list, one entry per
    step, of (rows, exp_avg, exp_avg_sq) as [n, 14] numpy arrays of `dtype`.
    manual: Adam written out here instead of torch.optim.Adam (the two agree,
    test_refine checks it); the bias_correction ablation needs it."""
    parts = _split(rows, dtype)
    n = parts[0].shape[0]
    s_chain = 1.0 if "render_scale" in ablate else float(s)
    manual = manual or "bias_correction" in ablate
    if manual:
        m = [torch.zeros_like(p) for p in parts]
        v = [torch.zeros_like(p) for p in parts]
    else:
        opt = torch.optim.Adam([dict(params=[p], lr=lrs[g]) for p, g in zip(parts, GROUPS)],
                               betas=betas, eps=eps, foreach=False)
    out = []
    for t, g in enumerate(np.asarray(grads), 1):
        G = torch.as_tensor(g, dtype=dtype)
        for p in parts:
            p.grad = None
        (activate(parts, s_chain, ablate) * G).sum().backward()
        if manual:
            b1 = 1.0 - betas[0] ** t
            b2s = (1.0 - betas[1] ** t) ** 0.5
            if "bias_correction" in ablate:
                b1 = b2s = 1.0
            with torch.no_grad():
                for p, mm, vv, grp in zip(parts, m, v, GROUPS):
                    mm.mul_(betas[0]).add_(p.grad, alpha=1.0 - betas[0])
                    vv.mul_(betas[1]).addcmul_(p.grad, p.grad, value=1.0 - betas[1])
                    p.addcdiv_(mm, vv.sqrt() / b2s + eps, value=-lrs[grp] / b1)
            ms, vs = m, v
        else:
            opt.step()
            ms = [opt.state[p]["exp_avg"] for p in parts]
            vs = [opt.state[p]["exp_avg_sq"] for p in parts]
        cat = lambda ts: torch.cat([x.detach() for x in ts], 1).numpy().copy()
        out.append((cat(parts), cat(ms), cat(vs)))
        assert out[-1][0].shape == (n, 14)
    return out


def chain_rule64(rows, act_grads, s):
    """The float64 chain rule alone: gradients of the packed activations
    [n, 14] -> gradient of the rows [n, 14]."""
    parts = _split(rows, torch.float64)
    (activate(parts, float(s)) * torch.as_tensor(np.asarray(act_grads), dtype=torch.float64)
     ).sum().backward()
    return torch.cat([p.grad for p in parts], 1).numpy()


def _row_norm_err(a, b):
    """max over rows of max_k |a - b| / max_k |b| (an all-zero reference row
    must be matched exactly)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num = np.abs(a - b).max(1)
    den = np.abs(b).max(1)
    e = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
    return float(e.max()) if len(e) else 0.0


def state_errors(got, ref, lrs=LRS):
    """{quantity.group: error} of one step's (rows, exp_avg, exp_avg_sq).
    p: max |a - b| / max(|ref|, lr) per entry -- the error of a parameter in
    units of its own size or of one step, whichever is larger.  m, v: per row,
    relative to the row's largest entry of the group."""
    out = {}
    for g in GROUPS:
        a, b = np.asarray(got[0], np.float64)[:, SL[g]], np.asarray(ref[0], np.float64)[:, SL[g]]
        out[f"p.{g}"] = float((np.abs(a - b) / np.maximum(np.abs(b), lrs[g])).max())
        out[f"m.{g}"] = _row_norm_err(np.asarray(got[1])[:, SL[g]], np.asarray(ref[1])[:, SL[g]])
        out[f"v.{g}"] = _row_norm_err(np.asarray(got[2])[:, SL[g]], np.asarray(ref[2])[:, SL[g]])
    return out


def act_errors(got, ref):
    return {f"act.{g}": _row_norm_err(np.asarray(got)[:, SL[g]], np.asarray(ref)[:, SL[g]])
            for g in GROUPS}


def run_errors(got_steps, ref_steps):
    """Worst state_errors over the steps."""
    worst = {}
    for a, b in zip(got_steps, ref_steps):
        for k, e in state_errors(a, b).items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst
