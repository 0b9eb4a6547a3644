"""The contracts of include/nerfloc_refine.h restated in numpy (fp64): the se(3) maps and the exponential's gradient, the rays of a pose and their backward,
the bilinear target, the masked loss and its cotangent, one refinement step (loss, latch, pose gradient, Adam) and the discard rule.  One pose at a time: the
library promises that a pose's bits do not depend on the other poses of a call."""
import numpy as np

EPS, COS_BOUND = 1e-4, 1e-4
STATE_DOUBLES = 44


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _mm(A, B):
    """The 3 x 3 product with every sum written out left to right, as the header states it (a BLAS product may fuse or reorder)."""
    return np.array([[A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)])


def _mv(A, x):
    return np.array([(A[i, 0] * x[0] + A[i, 1] * x[1]) + A[i, 2] * x[2] for i in range(3)])


def _coef(w):
    n = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = np.sqrt(max(n, EPS))
    inv, s, co = 1.0 / th, np.sin(th), np.cos(th)
    K = hat(w)
    return dict(n=n, th=th, f1=inv * s, f2=inv * inv * (1.0 - co), a=(1.0 - co) / (th * th), b=(th - s) / (th * th * th), K=K, K2=_mm(K, K))


def se3_exp(p):
    """(6) -> (4, 4)."""
    p = np.asarray(p, np.float64)
    c = _coef(p[3:])
    T = np.eye(4)
    T[:3, :3] = (np.eye(3) - c["f1"] * c["K"]) + c["f2"] * c["K2"]
    T[:3, 3] = _mv((np.eye(3) + c["a"] * c["K"]) + c["b"] * c["K2"], p[:3])
    return T


def se3_exp_backward(p, G):
    """d sum(G * exp(p)) / d p."""
    p, G = np.asarray(p, np.float64), np.asarray(G, np.float64)
    u, w = p[:3], p[3:]
    c = _coef(w)
    K, K2, GR, gt = c["K"], c["K2"], G[:3, :3], G[:3, 3]
    V = (np.eye(3) + c["a"] * K) + c["b"] * K2
    g_u = V.T @ gt
    outer = np.outer(gt, u)
    g_f1, g_f2, g_a, g_b = -(GR * K).sum(), (GR * K2).sum(), gt @ K @ u, gt @ K2 @ u
    GK2 = c["f2"] * GR + c["b"] * outer
    GK = c["a"] * outer - c["f1"] * GR + GK2 @ K.T + K.T @ GK2
    gw = np.array([GK[2, 1] - GK[1, 2], GK[0, 2] - GK[2, 0], GK[1, 0] - GK[0, 1]])
    if c["n"] >= EPS:   # torch.clamp's rule: the gradient passes where the input is not below the bound
        th, s, co = c["th"], np.sin(c["th"]), np.cos(c["th"])
        d_f1 = co / th - s / th ** 2
        d_f2 = s / th ** 2 - 2.0 * (1.0 - co) / th ** 3
        d_b = (1.0 - co) / th ** 3 - 3.0 * (th - s) / th ** 4
        g_th = g_f1 * d_f1 + (g_f2 + g_a) * d_f2 + g_b * d_b
        gw = gw + 2.0 * w * (g_th / (2.0 * th))
    return np.concatenate([g_u, gw])


def se3_log(T):
    """(4, 4) -> (6); the bottom row is not read."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3].T
    c = ((R[0, 0] + R[1, 1] + R[2, 2]) - 1.0) * 0.5
    bound = 1.0 - COS_BOUND
    slope = -1.0 / np.sqrt(1.0 - bound * bound)
    if c <= -bound:
        phi = (c + bound) * slope + np.arccos(-bound)
    elif c >= bound:
        phi = (c - bound) * slope + np.arccos(bound)
    else:
        phi = np.arccos(c)
    s = np.sin(phi)
    fac = phi / (2.0 * s) if abs(s) > 0.5 * EPS else 0.5 + phi * phi * (1.0 / 12)
    w = fac * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    k = _coef(w)
    V = (np.eye(3) + k["a"] * k["K"]) + k["b"] * k["K2"]
    t = T[:3, 3]
    C = np.array([[V[1, 1] * V[2, 2] - V[1, 2] * V[2, 1], V[1, 2] * V[2, 0] - V[1, 0] * V[2, 2], V[1, 0] * V[2, 1] - V[1, 1] * V[2, 0]],   # cofactors
                  [V[0, 2] * V[2, 1] - V[0, 1] * V[2, 2], V[0, 0] * V[2, 2] - V[0, 2] * V[2, 0], V[0, 1] * V[2, 0] - V[0, 0] * V[2, 1]],
                  [V[0, 1] * V[1, 2] - V[0, 2] * V[1, 1], V[0, 2] * V[1, 0] - V[0, 0] * V[1, 2], V[0, 0] * V[1, 1] - V[0, 1] * V[1, 0]]])
    det = (V[0, 0] * C[0, 0] + V[0, 1] * C[0, 1]) + V[0, 2] * C[0, 2]
    u = np.array([((C[0, j] * t[0] + C[1, j] * t[1]) + C[2, j] * t[2]) / det for j in range(3)])   # adjugate / determinant
    return np.concatenate([u, w])


# ---------------------------------------------------------------------------------------------- rays
def pixel_cams(K, uv):
    """(Rp, 3): ((x - cx) / fx, (y - cy) / fy, 1) of the pixels, coordinates truncated towards zero."""
    K = np.asarray(K, np.float32).astype(np.float64)
    xy = np.trunc(np.asarray(uv, np.float32).astype(np.float64))
    return np.stack([(xy[:, 0] - K[0, 2]) / K[0, 0], (xy[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(xy))], 1)


def pose_rays(T, K, uv):
    """-> rays_o, rays_d, centres (Rp, 3) fp64 (the library rounds them to fp32 on the store)."""
    cam = pixel_cams(K, uv)
    v = cam @ T[:3, :3].T
    d = v / np.sqrt((v * v).sum(1, keepdims=True))
    o = np.broadcast_to(T[:3, 3], d.shape).copy()
    return o, d, o.copy()


def pose_rays_backward(T, K, uv, g_o, g_d, g_c):
    """The (4, 4) cotangent of T (bottom row zero) of the ray chain."""
    cam = pixel_cams(K, uv)
    v = cam @ T[:3, :3].T
    ln = np.sqrt((v * v).sum(1, keepdims=True))
    dh = v / ln
    g_d = np.asarray(g_d, np.float64)
    g_v = (g_d - dh * (dh * g_d).sum(1, keepdims=True)) / ln
    G = np.zeros((4, 4))
    G[:3, :3] = g_v.T @ cam
    G[:3, 3] = (np.asarray(g_o, np.float64) + np.asarray(g_c, np.float64)).sum(0)
    return G


# ---------------------------------------------------------------------------------------------- target, loss
def _taps(x, n_in, n_out):
    src = np.maximum((x + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def sample_target(chw, H, W, uv):
    """chw (C, h, w) -> (Rp, C) fp64: the bilinear resize to (H, W) (align_corners=False) read at the pixels."""
    m = np.asarray(chw, np.float64)
    xy = np.trunc(np.asarray(uv, np.float32).astype(np.float64))
    x, y = np.clip(xy[:, 0], 0, W - 1), np.clip(xy[:, 1], 0, H - 1)
    x0, x1, lx0, lx1 = _taps(x, m.shape[2], W)
    y0, y1, ly0, ly1 = _taps(y, m.shape[1], H)
    return (ly0 * (lx0 * m[:, y0, x0] + lx1 * m[:, y0, x1]) + ly1 * (lx0 * m[:, y1, x0] + lx1 * m[:, y1, x1])).T


def loss_rows(out, mask, target):
    """One pose: out (Rp, C), mask (Rp), target (Rp, C) -> row_loss (Rp) fp64, g_out (Rp, C) fp64."""
    out, target, m = np.asarray(out, np.float64), np.asarray(target, np.float64), np.asarray(mask, np.float64)[:, None]
    e = (out - target) * m
    return (e * e).sum(1), 2.0 * m * e / (out.shape[0] * out.shape[1])


# ---------------------------------------------------------------------------------------------- the state of one pose, a step, the result
def init_state(pose):
    pose = np.asarray(pose, np.float64)
    return dict(params=se3_log(pose), m=np.zeros(6), v=np.zeros(6), grad=np.zeros(6), loss_init=0.0, loss_last=0.0, pose0=pose.copy(), t=0, nan=0)


def adam(s, g, lr, beta1, beta2, eps):
    """torch.optim.Adam's update of the six numbers, no weight decay."""
    s["t"] += 1
    s["m"] = s["m"] + (g - s["m"]) * (1.0 - beta1)
    s["v"] = s["v"] * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** s["t"], 1.0 - beta2 ** s["t"]
    s["params"] = s["params"] + (-(lr / bc1)) * (s["m"] / (np.sqrt(s["v"]) / np.sqrt(bc2) + eps))


def step(s, row_loss, C, g_o, g_d, g_c, K, uv, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    if s["nan"]:
        return
    loss = 0.0
    for v in np.asarray(row_loss, np.float64):
        loss += v
    loss = loss / (len(row_loss) * C)
    if s["t"] == 0:
        s["loss_init"] = loss
    s["loss_last"] = loss
    if np.isnan(loss):
        s["nan"] = 1
        return
    G = pose_rays_backward(se3_exp(s["params"]), K, uv, g_o, g_d, g_c)
    s["grad"] = se3_exp_backward(s["params"], G)
    adam(s, s["grad"], lr, beta1, beta2, eps)


def finish(s):
    """-> (T (4, 4), accepted)."""
    accepted = not (s["nan"] or s["loss_last"] > s["loss_init"])
    return (se3_exp(s["params"]) if accepted else s["pose0"].copy()), int(accepted)
