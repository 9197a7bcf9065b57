"""Float64 references, case generators and launch caps for the small kernels of the training step: the two losses,
Adam, the segmentation cross-entropy, the UNet's pool / upsample passes and the element-wise / gather kernels around
the fusion.  Plain torch on the CPU.  TEST infrastructure: tests/test_train_small_ops_cpu.py checks the references and
the generators without a GPU; tests/test_gpu_det_loss_fp64.py, test_gpu_loss_optim_fp64.py, test_gpu_resample_fp64.py
and test_gpu_elementwise_fp64.py compare the HIP kernels with them."""
import math

import torch
import torch.nn.functional as F

# ---- the grid caps: every one of these kernels is a grid-stride loop under a capped grid; above the cap a thread runs
# ---- a second iteration.  Items per pass = workgroups * 256 threads (or * 4 rows), from the launch lines named here.
DET_V4_CAP = 4096 * 256          # train_ops.hip :: dn_det_loss, grid_for(n * code / 4, 4096): float4s of loc (loop B)
DET_SCALAR_CAP = 2048 * 256      # train_ops.hip :: dn_det_loss, grid_for(n, 2048): anchors
ADAM_CAP = 4096 * 256            # train_ops.hip :: dn_adam_step, grid_for(n, 4096): elements
KD_ROWS_CAP = 8192 * 4           # train_ops.hip :: dn_kd_kl_loss, min(blocks, 8192) workgroups of 4 rows
SEG_CE_CAP = 2048 * 256          # seg_ops.hip :: dn_seg_ce_loss, min(.., 2048) workgroups: pixels
SEG_COUNT_CAP = 1024 * 256       # seg_ops.hip :: dn_seg_label_count, min(.., 1024) workgroups: pixels
RESAMPLE_CAP = 16384 * 256       # seg_ops.hip :: blocks_for: items of the pool / upsample kernels (NHWC and SP forms)
ELEMENTWISE_CAP = 8192 * 256     # train_ops.hip :: dn_add_rows / dn_upsample2_sum / dn_pair_add_ego / dn_pair_sum_ego, grid_for(total, 8192)

U32 = 2.0 ** -24                 # unit roundoff of float32 (round to nearest)
F32_MIN_NORMAL = 2.0 ** -126


# ---- detection loss --------------------------------------------------------------------------------------------------
# wrong-side logit gaps of the saturation sweep: dense around ln(1e30) = 69.08, where the clamped form broke, up to the
# point where its gradient was exactly zero (104), beyond, and one far outside anything exp() can represent
GAPS = [0.0, 1.0, 10.0, 30.0, 60.0, 69.0, 70.0, 75.0, 88.0, 100.0, 104.0, 120.0, 1e4]
SWEEP_BASES = [0.0, 0.0, -3.5, 1.25]      # the target logit of the four anchors of one sweep call
SWEEP_SIGNS = [1.0, -1.0, 1.0, -1.0]      # +: the OTHER logit is higher by `gap` (confidently wrong); -: lower


def det_takes_float4_path(n, code, *ptrs):
    """the dispatch rule of dn_det_loss: the float4 kernel for even n with n * code % 4 == 0 and 16-byte aligned tensors"""
    return n % 2 == 0 and (n * code) % 4 == 0 and all(p % 16 == 0 for p in ptrs)


def sweep_case(gap, fg, code=6, seed=0):
    """four anchors of one target class (fg: column 1, else column 0): target logit SWEEP_BASES[k], the other logit
    gap * SWEEP_SIGNS[k] above it.  All float32 (every value is exact in float32).  -> cls [4, 2], labels [4, 2],
    loc [4, code], targets [4, code], mask [4]"""
    g = torch.Generator().manual_seed(1000 + seed)
    zt = torch.tensor(SWEEP_BASES, dtype=torch.float32)
    zo = zt + torch.tensor(SWEEP_SIGNS, dtype=torch.float32) * float(gap)
    t = 1 if fg else 0
    cls = torch.zeros(4, 2)
    cls[:, t], cls[:, 1 - t] = zt, zo
    labels = torch.zeros(4, 2)
    labels[:, t] = 1.0
    loc = torch.randn(4, code, generator=g)
    targets = torch.randn(4, code, generator=g) * 0.5
    mask = torch.tensor([1.0, 0.0, 1.0, 1.0]) if fg else torch.zeros(4)
    return cls, labels, loc, targets, mask


def det_ref(cls, labels, loc, targets, mask, norm, alpha, gamma, sigma):
    """oracle.train_ref.det_loss in float64 under autograd -> (l_cls, l_loc, dcls, dloc), the gradients of l_cls + l_loc"""
    from oracle.train_ref import det_loss
    c = cls.double().clone().requires_grad_(True)
    l = loc.double().clone().requires_grad_(True)
    l_cls, l_loc = det_loss({"cls": c, "loc": l}, labels.double(), targets.double(), mask.double(), norm=norm,
                            alpha=alpha, gamma=gamma, sigma=sigma)
    (l_cls + l_loc).backward()
    return float(l_cls.detach()), float(l_loc.detach()), c.grad, l.grad


def focal_grad_scale(labels, alpha, norm):
    """a_t / norm per anchor: the magnitude the class gradient saturates at (0 for a "don't care" row)"""
    fg = labels[:, 1] > 0.5
    care = fg | (labels[:, 0] > 0.5)
    a = torch.where(fg, torch.full((labels.shape[0],), float(alpha)), torch.full((labels.shape[0],), 1.0 - float(alpha)))
    return (a * care).double() / norm


def smooth_l1_edge_case(sigma, code, big):
    """residuals loc - targets (targets = 0, so the residual is the float32 value itself): 0, -0, +-1/sigma^2 as float32,
    their float32 neighbours on both sides, a few ordinary ones and, with `big`, +-1e6 and 3e30; every residual once
    under mask 1 and once under mask 0.  -> cls, labels, loc, targets, mask with n a multiple of 4"""
    t = torch.tensor(1.0 / (sigma * sigma), dtype=torch.float32)
    inf = torch.tensor(float("inf"))
    vals = [torch.tensor(0.0), torch.tensor(-0.0)]
    for s in (1.0, -1.0):
        vals += [s * t, s * torch.nextafter(t, inf), s * torch.nextafter(t, -inf)]
    vals += [torch.tensor(v) for v in (0.03, -0.07, 0.5, -2.25, 17.0)]
    if big:
        vals += [torch.tensor(v) for v in (1e6, -1e6, 3e30)]
    vals = torch.stack([v.float() for v in vals])
    rows = -(-vals.numel() // code)
    rows += (-rows) % 2                                   # both masks -> n = 2 * rows, a multiple of 4
    flat = torch.zeros(rows * code)
    flat[:vals.numel()] = vals
    flat[vals.numel():] = 0.25
    loc = torch.cat([flat.view(rows, code), flat.view(rows, code)])
    n = 2 * rows
    mask = torch.cat([torch.ones(rows), torch.zeros(rows)])
    g = torch.Generator().manual_seed(77)
    cls = torch.randn(n, 2, generator=g) * 3
    fg = torch.arange(n) % 3 == 0
    labels = torch.stack([(~fg).float(), fg.float()], -1)
    labels[1] = 0
    return cls, labels, loc, torch.zeros(n, code), mask


LONG_DET_N = 2 * 256 * 256 * 6      # two 256 x 256 maps of 6 anchors


def long_det_case():
    """786 432 anchors, code 6, ~5 % foreground, ~2 % ignored, logits randn * 3 with 1 % of the rows given a gap drawn
    from the sweep (either sign).  float32 tensors."""
    g = torch.Generator().manual_seed(60)
    n, code = LONG_DET_N, 6
    cls = torch.randn(n, 2, generator=g) * 3
    fg = torch.rand(n, generator=g) < 0.05
    ignore = torch.rand(n, generator=g) < 0.02
    sat = (torch.rand(n, generator=g) < 0.01).nonzero().flatten()
    gap = torch.tensor(GAPS, dtype=torch.float32)[torch.randint(0, len(GAPS), (sat.numel(),), generator=g)]
    sign = torch.randint(0, 2, (sat.numel(),), generator=g).float() * 2 - 1
    cls[sat, 1] = cls[sat, 0] + sign * gap
    labels = torch.stack([(~fg).float(), fg.float()], -1)
    labels[ignore] = 0
    loc = torch.randn(n, code, generator=g)
    targets = torch.randn(n, code, generator=g) * 0.5
    return cls, labels, loc, targets, fg.float(), sat


def unaligned_copy(t):
    """the same values in a view whose data pointer is 8 bytes past a 16-byte boundary (what the existing test builds)"""
    pad = torch.zeros(t.numel() + 2, dtype=t.dtype, device=t.device)
    pad[2:] = t.reshape(-1)
    v = pad[2:].view(t.shape)
    assert v.data_ptr() % 16 == 8
    return v


# ---- knowledge distillation -------------------------------------------------------------------------------------------
def kd_ref(student, teacher, kd_weight, norm_rows=None):
    """kd_weight * KLDiv(log_softmax(s), softmax(t)) with reduction "mean" (over all elements) in float64, the mean taken
    over norm_rows rows when given -> (term, d term / d student)"""
    c = student.shape[-1]
    s = student.double().reshape(-1, c).clone().requires_grad_(True)
    t = teacher.double().reshape(-1, c)
    term = kd_weight * F.kl_div(F.log_softmax(s, 1), F.softmax(t, 1), reduction="mean")
    if norm_rows is not None:
        term = term * (s.shape[0] / float(norm_rows))
    term.backward()
    return float(term.detach()), s.grad.reshape(student.shape)


def kd_case(rows, c, seed):
    """student / teacher [rows, c] = randn * 3 with special rows: 0 student gap 200 (one logit 200 above the rest),
    1 teacher gap 200 (its other probabilities underflow to 0 in float32), 2 both on different channels, 3 a logit 200
    BELOW the rest in both, 4 / 5 all-equal logits (student / both)"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, c, generator=g) * 3
    t = torch.randn(rows, c, generator=g) * 3
    k = lambda r: r % rows
    s[k(0), 0] += 200.0
    t[k(1), c - 1] += 200.0
    s[k(2), 0] += 200.0
    t[k(2), c // 2] += 200.0
    s[k(3), c - 1] -= 200.0
    t[k(3), 0] -= 200.0
    s[k(4)] = 1.5
    s[k(5)] = -2.0
    t[k(5)] = 7.0
    return s, t


# ---- Adam ---------------------------------------------------------------------------------------------------------------
def adam64(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """one torch.optim.Adam step (no amsgrad, L2 weight decay added to the gradient) restated in float64 on the values
    given -> (p_new, m_new, v_new), float64"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    b1, b2 = betas
    if weight_decay != 0.0:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adam_torch(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """the same step by torch.optim.Adam itself in the dtype of p, from the given state -> (p_new, m_new, v_new)"""
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g.clone()
    opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


ADAM_N = 1048576 + 4099      # one full pass of the capped grid and a partial one


def adam_case(n=ADAM_N, seed=5):
    """float32 p (weights of kaiming size), m, v and a gradient mixing entries of exactly 0 (on v = 0 and m = 0), of 1e-20
    (the square underflows), of +-1e15 and of O(1)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.02
    grad = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01 + 1e-4
    kind = torch.arange(n) % 16
    grad[kind == 3] = 0.0
    m[kind == 3] = 0.0
    v[kind == 3] = 0.0
    grad[kind == 5] = 1e-20
    grad[kind == 7] = 1e15
    grad[kind == 9] = -1e15
    return p, grad, m, v


def adam_mv_bounds(p, g, m, v, betas, weight_decay):
    """absolute bounds on |m_kernel - m_64| and |v_kernel - v_64| from the operand magnitudes, u = 2^-24; see
    test_gpu_loss_optim_fp64.py :: test_adam_step_matches_float64 for the derivation"""
    b1, b2 = betas
    G = g.double().abs() + abs(weight_decay) * p.double().abs()
    floor = 4 * F32_MIN_NORMAL
    bm = U32 * (3 * m.double().abs() + (0.5 + 6 * (1 - b1)) * G) + floor
    bv = U32 * (3 * v.double().abs() + (0.5 + 10 * (1 - b2)) * G * G) + floor
    return bm, bv


ADAM_GRID = [(wd, eps) for wd in (0.0, 1e-4) for eps in (1e-8, 1e-3)]
ADAM_STEPS = [1, 2, 3, 5000]      # 1-3 chained from zero state, 5000 from adam_case()'s m, v


def adam_grad(grad, step):
    """the gradient of step `step`: adam_case()'s, a decade smaller / larger at steps 1 / 3"""
    return grad * {1: 0.1, 3: 10.0}.get(step, 1.0)


# MEASURED, not derived: the largest |update_f32 - update_64| (update = p_new - p_old, in float64 from the float32 values) of
# torch's own float32 CPU Adam against adam64 over adam_case(), ADAM_GRID and ADAM_STEPS is 4.363e-9 (it is the rounding of
# p_new, |p| < 0.12: half an ulp is 3.7e-9, plus the float32 arithmetic of an update of up to 2.8e-2);
# tests/test_train_small_ops_cpu.py re-measures it.  The kernel is allowed four times that: another, legitimate, order
# of the same operations.
ADAM_UPDATE_DEV_MEASURED = 4.4e-9
ADAM_UPDATE_BOUND = 4 * ADAM_UPDATE_DEV_MEASURED


# ---- segmentation cross-entropy -------------------------------------------------------------------------------------------
SEG_PIXELS = (1, 600, 1000)      # 600 000 pixels


def seg_case(classes, shape=SEG_PIXELS, ignored=0.3, seed=0):
    """logits [*shape, classes] = randn * 3 with every 1000th pixel given a logit gap of 1e4 (up on one class, down on
    another when there is one), int64 labels with `ignored` of them -100"""
    g = torch.Generator().manual_seed(200 + classes + seed)
    z = torch.randn(*shape, classes, generator=g) * 3
    y = torch.randint(0, classes, shape, generator=g)
    flat = z.view(-1, classes)
    rows = torch.arange(0, flat.shape[0], 1000)
    flat[rows, rows % classes] += 1e4
    flat[rows + 1, (rows + 1) % classes] -= 1e4
    y[torch.rand(shape, generator=g) < ignored] = -100
    return z, y


def seg_ref(z, y):
    """F.cross_entropy (mean over the live pixels) in float64 -> (loss, dlogits)"""
    c = z.shape[-1]
    zd = z.double().reshape(-1, c).clone().requires_grad_(True)
    loss = F.cross_entropy(zd, y.reshape(-1))
    loss.backward()
    return float(loss.detach()), zd.grad.reshape(z.shape)


# ---- pool / upsample ----------------------------------------------------------------------------------------------------------
UPSAMPLE_SIZES = [(h, w) for h in (1, 2, 3, 5, 8, 31, 64) for w in (1, 2, 7, 33)]


def upsample_ref(x_nhwc, dy_nhwc=None):
    """F.interpolate(x2, bilinear, align_corners=True) in float64 on an NHWC map -> y NHWC (and dx NHWC for dy)"""
    x = x_nhwc.double().permute(0, 3, 1, 2).clone().requires_grad_(dy_nhwc is not None)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    if dy_nhwc is None:
        return y.permute(0, 2, 3, 1)
    y.backward(dy_nhwc.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1)


def maxpool_aten(x_nhwc, dy_nhwc=None):
    """ATen's MaxPool2d(2) on the CPU (contiguous NCHW float32) -> y NHWC (and dx NHWC for dy)"""
    x = x_nhwc.permute(0, 3, 1, 2).contiguous().clone().requires_grad_(dy_nhwc is not None)
    y = F.max_pool2d(x, 2)
    if dy_nhwc is None:
        return y.permute(0, 2, 3, 1).contiguous()
    y.backward(dy_nhwc.permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1).contiguous(), x.grad.permute(0, 2, 3, 1).contiguous()


def maxpool_rule(x_nhwc):
    """the documented rule, restated without ATen: scan the window in the order (0,0) (0,1) (1,0) (1,1) and take
    val when val > max or isnan(val) -> (y NHWC, arg NHWC int64 in 0..3)"""
    n, h, w, c = x_nhwc.shape
    win = x_nhwc.view(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    best = win[..., 0].clone()
    arg = torch.zeros(best.shape, dtype=torch.int64)
    for k in range(1, 4):
        v = win[..., k]
        take = (v > best) | torch.isnan(v)
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return best, arg


POOL_SPECIALS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def pool_special_windows():
    """-> [(name, [4 values])]: every special value at every window position, several NaNs, +-0 ties, all-equal windows"""
    nan, inf = float("nan"), float("inf")
    out = []
    for name, s in POOL_SPECIALS.items():
        for pos in range(4):
            wdw = [0.5, -1.25, 2.0, -0.75]
            wdw[pos] = s
            out.append(("%s@%d" % (name, pos), wdw))
    out += [("nan,nan", [nan, 3.0, nan, 1.0]), ("nan,+inf", [inf, nan, 1.0, inf]), ("all nan", [nan] * 4),
            ("+inf,+inf", [1.0, inf, inf, 0.0]), ("+inf,-inf", [-inf, inf, -inf, 2.0]), ("all -inf", [-inf] * 4)]
    for pos in range(4):                      # +0 / -0 ties over negatives: the first zero in scan order wins, whatever its sign
        a = [-1.0] * 4
        a[pos] = -0.0
        a[(pos + 1) % 4] = 0.0
        out.append(("-0@%d,+0@%d" % (pos, (pos + 1) % 4), a))
    out += [("all +0", [0.0] * 4), ("all -0", [-0.0] * 4), ("-0,+0,-0,+0", [-0.0, 0.0, -0.0, 0.0]),
            ("all 1.5", [1.5] * 4), ("all -2", [-2.0] * 4), ("max twice", [3.0, 1.0, 3.0, 2.0])]
    return out


def pool_special_map(c=8):
    """an NHWC float32 map [2, 2 * rows, 16, c] whose 2 x 2 windows cycle through pool_special_windows() (shifted by
    channel and image so that every channel lane of a float4 meets every window), ordinary windows in between"""
    wins = pool_special_windows()
    per_row = 8
    rows = -(-2 * len(wins) // per_row)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 2 * rows, 2 * per_row, c, generator=g)
    for img in range(2):
        for ch in range(c):
            for k in range(rows * per_row):
                if k % 2:
                    continue
                oy, ox = divmod(k, per_row)
                vals = wins[(k // 2 + ch + 3 * img) % len(wins)][1]
                for pos in range(4):
                    x[img, 2 * oy + pos // 2, 2 * ox + pos % 2, ch] = vals[pos]
    return x


def bits(t):
    """bit patterns, for comparisons that must see NaN and the sign of zero"""
    return t.contiguous().view(torch.int32)


# ---- the fusion's weighted sum ----------------------------------------------------------------------------------------------
def fuse_combine_ref(z4, maps, lists, ego_out, dfused):
    """float64 autograd reference of dn_fuse_combine / _backward: per ego list of (pair, map) entries, weights =
    softmax over the list of relu(z4[pair]) (0 for pair < 0), fused = sum of weights * maps[map].
    z4 [P, h, w, 1], maps [M, h, w, c], dfused [E, h, w, c] -> (fused per list, weights per list, dmaps, dz4)"""
    z = z4.double().clone().requires_grad_(True)
    mp = maps.double().clone().requires_grad_(True)
    h, w = maps.shape[1], maps.shape[2]
    outs, wts = [], []
    for lst in lists:
        s = torch.stack([F.relu(z[p, ..., 0]) if p >= 0 else torch.zeros(h, w, dtype=torch.float64) for p, _ in lst])
        wk = torch.softmax(s, 0)
        wts.append(wk.detach())
        outs.append(sum(wk[k].unsqueeze(-1) * mp[mi] for k, (_, mi) in enumerate(lst)))
    loss = sum((o * dfused[eo].double()).sum() for o, eo in zip(outs, ego_out))
    loss.backward()
    return [o.detach() for o in outs], wts, mp.grad, z.grad


# lengths 1, 2, 6; a pair index of -1 (an entry without a logit: an ego that is not live) is a list's only entry, as train.py builds it
FUSE_LISTS = [[(-1, 0)], [(0, 1), (1, 2)], [(2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]]
FUSE_EGO_OUT = [2, 0, 3]
FUSE_MAPS = 10                      # map 9 belongs to no list
FUSE_HW = (5, 7)                    # 3 egos x 35 pixels = 105 items: the last workgroup of 4 holds one


def fuse_case(c, seed=0):
    """z4 [8, 5, 7, 1] with negative entries, exact zeros and 80s among randn * 2; maps [10, 5, 7, c]; dfused [4, 5, 7, c]"""
    g = torch.Generator().manual_seed(300 + c + seed)
    h, w = FUSE_HW
    z4 = torch.randn(8, h, w, 1, generator=g) * 2
    flat = z4.view(8, -1)
    flat[:, 0] = 0.0
    flat[0, 3] = 80.0
    flat[2, 5] = 80.0
    flat[3, 5] = 80.0
    flat[4, 7] = 80.0
    flat[1, 9] = -80.0
    flat[6, 7] = 80.0                   # two 80s in one list at one pixel: weights of 1/2
    maps = torch.randn(FUSE_MAPS, h, w, c, generator=g)
    dfused = torch.randn(4, h, w, c, generator=g)
    return z4, maps, dfused
