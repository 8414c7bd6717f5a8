"""Shared by the suites of the batched DETR baselines (``csrc/detr_baselines.hip``): the case table, the slabs of a case, a float64
restatement of the three methods in the reference's own MATRIX form -- the full ``compute_rollout_attention`` products
(DETR/modules/ExplanationGenerator.py:5-16), ``R_q_q^T . (cam_q_i . R_i_i)`` (:240-273), the head mean (:226-238) and the GradCAM map
(:275-305), and only then the pick of row ``targets[k]`` -- so that it shares no algebra with the row-vector form the kernels use, and
per-case error bounds COUNTED from the kernels' summation orders.

A case is ``(Ni, Q, H, K, n_enc, n_dec)``.  Slabs are softmax rows of ``2 * randn`` logits (fp32); gradients are ``randn + c_h`` with a
per-head offset ``c_h`` of either sign, per target ``[K, H, Q, Ni]`` and one shared slab ``[H, Q, Ni]``; nothing in them is zero
outside row ``t_k``.

The bounds.  u = 2^-24, gamma(c) = c u / (1 - c u).  Every operation of the kernels is one fp32 add, multiply, divide or FMA, each
with relative error <= u.

raw attention: heads added in order (H - 1 adds) and one division: c = H.  All terms are >= 0, so |err[j]| <= gamma(H) ref[j].

rollout: all terms are >= 0, so |err[j]| <= gamma(c) ref[j] with c the number of roundings on the deepest path:
  head mean of any slab                       H                       (H - 1 adds, one division)
  decoder layer  y <- (B y + y) / r           2 H + 18                dot: H (B~) + 2 (a multiply and an FMA per lane) + 6 (xor tree);
                                                                      + y: 1; r = 1 + rowsum: H + 1 (lane add) + 6 (tree) + 1; division: 1
  s = u^T P~_x                                H + Q                   an FMA per query, in order
  encoder layer  x <- w A~ + w, w = x / r     2 H + ceil(Ni / 64) + 16 + ceil(Ni / 8)
                                                                      r = 1 + rowsum: H + ceil(Ni / 64) (lane adds) + 6 (tree) + 1;
                                                                      w: 1; the strip's FMAs: H (A~) + 8; the strips in order:
                                                                      ceil(Ni / 8) - 1; + w[j]: 1
  c = n_dec (2 H + 18) + H + Q + n_enc (2 H + ceil(Ni / 64) + 16 + ceil(Ni / 8)).

GradCAM: w sums signed values.  Its depth: 8 chunk adds per thread, 2 for the four components, 6 for the xor tree, 2 for the four
waves, S - 1 for the S = ceil(Q Ni / 8192) strips and the division: d = 18 + S, so |w^[h] - w[h]| <= gamma(d) sum|grad[h]| / (Q Ni) =: e[h].
The map is one multiply, H - 1 FMAs and one division, then the clamp (which cannot grow an error):
|err[j]| <= (sum_h P[h, t, j] e[h] (1 + gamma(H + 1)) + gamma(H + 1) sum_h P[h, t, j] |w[h]|) / H."""
import numpy as np

U = 2.0 ** -24
STEP_ROWS = 8            # rows of a vector-matrix strip (kDbStepRows)
GRAD_STRIP = 8192        # floats of a gradient strip (kDcStrip)

#        Ni   Q    H  K   n_enc n_dec
CASES = ((1, 1, 1, 1, 1, 1),
         (2, 2, 3, 2, 2, 1),
         (5, 7, 8, 5, 1, 2),
         (63, 100, 3, 17, 6, 2),
         (64, 128, 1, 2, 2, 6),
         (65, 7, 8, 5, 6, 6),
         (255, 100, 3, 1, 2, 2),
         (257, 128, 8, 17, 6, 1))
FULL = (950, 100, 8, 16, 6, 6)       # detr_resnet50_head on 25 x 38 features


def case_id(case):
    return "Ni%d-Q%d-H%d-K%d-enc%d-dec%d" % tuple(case)


def gamma(c):
    return c * U / (1.0 - c * U)


def targets_of(case):
    """0, Q - 1 and repeats among them; the pattern starts at another place for every case, so K = 1 meets both ends of the range."""
    Ni, Q, H, K, n_enc, n_dec = case
    base = [0, Q - 1, Q // 2, Q - 1, min(1, Q - 1), 0]
    start = (Ni + K) % len(base)
    return np.array([base[(start + i) % len(base)] for i in range(K)], dtype=np.int64)


def _softmax(rng, shape):
    z = rng.standard_normal(shape, dtype=np.float32) * 2.0
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def make_case(case, seed=0):
    Ni, Q, H, K, n_enc, n_dec = case
    rng = np.random.default_rng(1000 + seed + 7 * Ni + Q)
    c = dict(Ni=Ni, Q=Q, H=H, K=K, targets=targets_of(case))
    c["grad"] = (rng.standard_normal((K, H, Q, Ni), dtype=np.float32)
                 + rng.standard_normal((K, H, 1, 1), dtype=np.float32)).astype(np.float32)
    c["grad_shared"] = (rng.standard_normal((H, Q, Ni), dtype=np.float32) + rng.standard_normal((H, 1, 1), dtype=np.float32)).astype(np.float32)
    c["cross"] = _softmax(rng, (H, Q, Ni))
    c["dec"] = [_softmax(rng, (H, Q, Q)) for _ in range(n_dec)]
    c["enc"] = [_softmax(rng, (H, Ni, Ni)) for _ in range(n_enc)]
    return c


# ---------------------------------------------------------------------------------------- float64 restatement, matrix form
def compute_rollout_attention64(mats):
    """:5-16: add I, divide every row by its sum, left-multiply from the first matrix up."""
    eye = np.eye(mats[0].shape[-1])
    mats = [m + eye for m in mats]
    mats = [m / m.sum(axis=-1, keepdims=True) for m in mats]
    joint = mats[0]
    for m in mats[1:]:
        joint = m @ joint
    return joint


def head_mean64(slab):
    return slab.astype(np.float64).mean(axis=0)


def raw64(cross, targets):
    """:226-238 -> ``(ref [K, Ni], bound [K, Ni])``."""
    ref = head_mean64(cross)[np.asarray(targets)]
    return ref, gamma(cross.shape[0]) * ref


def rollout_depth(H, Q, Ni, n_enc, n_dec):
    strips = (Ni + STEP_ROWS - 1) // STEP_ROWS
    return n_dec * (2 * H + 18) + H + Q + n_enc * (2 * H + (Ni + 63) // 64 + 2 * STEP_ROWS + strips)


def rollout64(enc, dec, cross, targets):
    """:240-273 -> ``(ref [K, Ni], bound [K, Ni])``: the whole ``R_q_i`` first, then its rows."""
    R_ii = compute_rollout_attention64([head_mean64(a) for a in enc])
    R_qq = compute_rollout_attention64([head_mean64(b) for b in dec])
    R_qi = R_qq.T @ (head_mean64(cross) @ R_ii)
    ref = R_qi[np.asarray(targets)]
    H, Q, Ni = cross.shape
    return ref, gamma(rollout_depth(H, Q, Ni, len(enc), len(dec))) * ref


def gradcam_depth(Q, Ni):
    return 18 + (Q * Ni + GRAD_STRIP - 1) // GRAD_STRIP


def gradcam64(cross, grad, targets, clamp=True):
    """:275-305 for every target.  ``grad``: ``[K, H, Q, Ni]`` or one shared ``[H, Q, Ni]`` -> ``(ref [K, Ni], bound [K, Ni])``."""
    targets = np.asarray(targets)
    H, Q, Ni = cross.shape
    P = cross.astype(np.float64)
    ref = np.zeros((len(targets), Ni))
    bound = np.zeros_like(ref)
    gH = gamma(H + 1)
    for k, t in enumerate(targets):
        g = (grad if grad.ndim == 3 else grad[k]).astype(np.float64)
        w = g.mean(axis=(1, 2), keepdims=True)                                   # grad.mean([1, 2], keepdim=True)
        cam = (P * w).mean(axis=0)                                                # [Q, Ni]
        ref[k] = (np.maximum(cam, 0.0) if clamp else cam)[t]
        e = gamma(gradcam_depth(Q, Ni)) * np.abs(g).sum(axis=(1, 2)) / (Q * Ni)   # [H]
        bound[k] = ((P[:, t, :] * e[:, None]).sum(0) * (1.0 + gH) + gH * (P[:, t, :] * np.abs(w[:, 0, :])).sum(0)) / H
    return ref, bound
