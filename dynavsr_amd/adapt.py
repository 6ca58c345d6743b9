"""The per-frame test-time adaptation of DynaVSR as one reusable function.

This is the body of the hot loop of codes/test_dynavsr.py:197-283 (and of the validation loops
train_dynavsr.py:552-677) expressed over the wrapper API, so that drivers, benchmarks and tests
share one implementation:

    baseline SR  ->  deepcopy(netG, netE)  ->  inner optimizer over G u E params
    for adapt_iter steps:  SLR = netE(LR) (with grad);  loss = cri(netG(SLR), LR[:,center])
                           + 10 * L1(SLR, netE_fixed(LR));  backward;  step
    adapted SR = netG(LR)

One deviation that the wrapper contract allows and SURVEY.md §8f-1 calls out: the frozen
estimator's output does not change inside the step loop, so it is computed once per frame.
"""
from copy import deepcopy

import math
import os

import torch
import torch.nn.functional as F

from . import engine, hipops, optim


def make_inner_optimizer(opt, netG, netE):
    m = opt['train']['maml']
    params = [p for p in netG.parameters() if p.requires_grad]
    if not opt['train']['use_real']:
        params += [p for p in netE.parameters() if p.requires_grad]
    # same update rules as the torch.optim objects test_dynavsr.py:223-231 builds; on the GPU the 158
    # parameter tensors are stepped by the native multi-tensor kernels (dynavsr_amd/optim.py)
    on_gpu = all(p.is_cuda for p in params)
    if m['optimizer'] == 'Adam':
        if on_gpu:
            return optim.Adam(params, lr=m['lr_alpha'], betas=(m['beta1'], m['beta2']))
        return torch.optim.Adam(params, lr=m['lr_alpha'], betas=(m['beta1'], m['beta2']))
    if m['optimizer'] == 'SGD':
        if on_gpu:
            return optim.SGD(params, lr=m['lr_alpha'])
        return torch.optim.SGD(params, lr=m['lr_alpha'])
    raise NotImplementedError()


def backbone_input(opt, clip):
    """What the drivers feed netG: the clip itself for EDVR / DUF; for TOFlow, which works at the output size, the
    clip brought there by F.interpolate(scale_factor=scale, mode='bicubic', align_corners=True)
    (test_dynavsr.py:188-193, 245-250) -- one native launch (tofops.upsample_bicubic_ac), differentiable."""
    if (opt['network_G'] or {}).get('which_model_G') == 'TOF' and clip.is_cuda:
        from . import tofops
        return tofops.upsample_bicubic_ac(clip, opt['scale'])
    if (opt['network_G'] or {}).get('which_model_G') == 'TOF':
        b, t, c, h, w = clip.shape
        up = F.interpolate(clip.reshape(b * t, c, h, w), scale_factor=opt['scale'], mode='bicubic', align_corners=True)
        return up.reshape(b, t, c, h * opt['scale'], w * opt['scale'])
    return clip


def draw_patch_positions(min_h, min_w, ps, n):
    """n x common_crop's draw (preprocessing.py:76-77): py = randrange(min_h - ps + 1), then px, per patch."""
    import random
    py, px = [], []
    for _ in range(n):
        py.append(random.randrange(0, min_h - ps + 1))
        px.append(random.randrange(0, min_w - ps + 1))
    return py, px


def slr_region(region, scale):
    """The SLR cells that hold at least one real pixel of a clip whose valid LR size is region = (h, w):
    (ceil(h / scale), ceil(w / scale)) -- the region of the SLR term."""
    s = int(scale)
    return -(-int(region[0]) // s), -(-int(region[1]) // s)


def patch_region(region, scale):
    """The SLR cells that hold real pixels alone: (floor(h / scale), floor(w / scale)) -- where use_patch draws its patches."""
    s = int(scale)
    return int(region[0]) // s, int(region[1]) // s


def check_adapt_region(opt, lqs_shape, region):
    """The `region` argument of the adaptation loops for a clip [..., H, W]: None, or (h, w) with 1 <= h <= H, 1 <= w <= W, the
    clip's valid LR size (the rest is padding).  Returns None for None and for the whole clip -- the calls of before -- and
    (h, w) otherwise; with train.maml.use_patch the region must hold one patch (ValueError).  Host code."""
    if region is None:
        return None
    h, w = hipops.check_region(lqs_shape, region, "region")
    if (h, w) == (int(lqs_shape[-2]), int(lqs_shape[-1])):
        return None
    m = opt['train']['maml']
    if m['use_patch']:
        # (TOFlow sees the SLR clip at the clip's own size, backbone_input: its patches are cut there, one cell per pixel)
        k = 1 if (opt['network_G'] or {}).get('which_model_G') == 'TOF' else opt['scale']
        ps, (ph, pw) = int(m['patch_size']) // 2, patch_region((h, w), k)
        if (opt['network_G'] or {}).get('which_model_G') == 'EDVR' and ps % 4:
            raise ValueError("train.maml.patch_size=%d cuts patches of %d x %d (patch_size // 2), and EDVR takes multiples of 4"
                             % (m['patch_size'], ps, ps))
        if ph < ps or pw < ps:
            raise ValueError("region=%r holds %d x %d whole cells of the backbone's input (1 / %d the size), fewer than a patch "
                             "of %d x %d (train.maml.patch_size=%d: the crop's edge is patch_size // 2)" % (
                                 (h, w), ph, pw, k, ps, ps, m['patch_size']))
    return h, w


def crop(LR_seq, HR, num_patches_for_batch=4, patch_size=44, region=None):
    """The `crop` of test_dynavsr.py:118-145 / train_dynavsr.py:208-243: `num_patches_for_batch` random patches of the
    SLR clip LR_seq [1,T,C,h,w] and, at the same places, of its target HR [1,C,s*h,s*w], stacked into batches
    [P,T,C,ps,ps] / [P,C,s*ps,s*ps] with ps = patch_size // 2.  Positions come from python's `random` in the
    reference's order (common_crop, preprocessing.py:76-77: py then px per patch), so a seeded run draws the same
    patches; the crops themselves are one gather launch each (hipops.patch_gather), differentiable w.r.t. the clip.
    region = (h, w): only the top-left h x w of HR is real (the rest is padding), and the patches are drawn where they cover
    real pixels alone -- positions below (floor(h / k), floor(w / k)) for HR k times the size of the smaller tensor."""
    assert HR.size(0) == 1
    seq, hr = LR_seq[0], HR[0]
    min_h, min_w = min(seq.shape[-2], hr.shape[-2]), min(seq.shape[-1], hr.shape[-1])
    ps = patch_size // 2
    s_seq, s_hr = int(seq.shape[-2] // min_h), int(hr.shape[-2] // min_h)
    if region is not None:
        min_h, min_w = min(min_h, int(region[0]) // s_hr), min(min_w, int(region[1]) // s_hr)
        if min_h < ps or min_w < ps:
            raise ValueError("crop: region=%r leaves %d x %d positions, fewer than a patch of %d x %d" % (
                tuple(region), min_h, min_w, ps, ps))
    py, px = draw_patch_positions(min_h, min_w, ps, num_patches_for_batch)
    return (hipops.patch_gather(seq, py, px, ps, s_seq), hipops.patch_gather(hr, py, px, ps, s_hr))


def _fresh_copy(dst, src):
    """dst = deepcopy(src) (test_dynavsr.py:208).  When dst already is a copy from the previous frame (same class,
    same parameter names and shapes, same device) only the values are refreshed: one multi-tensor copy instead of
    re-creating ~150 modules and parameters (2.9 -> 0.3 ms per frame for netG + netE)."""
    if dst is not None and dst is not src and type(dst) is type(src):
        d, s = list(dst.named_parameters()), list(src.named_parameters())
        same = len(d) == len(s) and not list(src.buffers()) and all(
            a[0] == b[0] and a[1].shape == b[1].shape and a[1].device == b[1].device and a[1].dtype == b[1].dtype
            and a[1].requires_grad == b[1].requires_grad for a, b in zip(d, s))
        if same:
            with torch.no_grad():
                torch._foreach_copy_([a[1] for a in d], [b[1] for b in s])
            for _, p in d:
                p.grad = None
            dst.train(src.training)
            return dst
    return deepcopy(src)


def adapt_frame(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, val_data, slr_weight=10.0,
                final_test=True, region=None):
    """Adapt copies of (model.netG, est_model.netE) on one LR clip and super-resolve it.

    val_data: {'LQs': [1,N,3,H,W] (+ 'SuperLQs' when train.use_real)}.  Returns a dict with the
    adapted output ``sr`` [1,3,sH,sW] (on device), the per-step ``losses`` and the updated wrappers
    (modelcp.netG / est_modelcp.netE hold the adapted weights).

    region = (h, w): the clip's valid LR size -- a frame of h x w that was padded at the bottom and right to H x W.  The
    objective then counts the frame's own pixels: the pixel loss is the mean over [:h, :w] of netG(SLR) and the LR centre
    frame (hipops.charbonnier_region; any other criterion on the two slices), the SLR term the mean over the
    slr_region(region, scale) cells that hold a real pixel (hipops.inner_loss_region), and use_patch draws its patches inside
    patch_region(region, scale), where the pixel loss needs no mask (the SLR term keeps its region).  The networks still run
    on the whole padded clip, and ``sr`` is the whole [1,3,sH,sW].  None, or the whole clip, is every call of before."""
    lqs = val_data['LQs']
    assert lqs.size(0) == 1
    region = check_adapt_region(opt, lqs.shape, region)
    center = lqs.size(1) // 2
    steps = opt['train']['maml']['adapt_iter']
    prev = (modelcp.netG, est_modelcp.netE)
    modelcp.netG, est_modelcp.netE = _fresh_copy(modelcp.netG, model.netG), _fresh_copy(est_modelcp.netE, est_model.netE)
    # a new inner optimiser per frame, like the reference; when the copies were refreshed in place the previous
    # frame's native optimiser holds the very same parameters and is reset instead of rebuilt
    m = opt['train']['maml']
    sig = (m['optimizer'], m['lr_alpha'], m.get('beta1'), m.get('beta2'), bool(opt['train']['use_real']),
           tuple(id(p) for p in modelcp.netG.parameters()), tuple(id(p) for p in est_modelcp.netE.parameters()))
    cached = getattr(modelcp, '_inner_opt', None)
    # (the signature holds the identity of every parameter: a cached optimiser is only reused for the very tensors
    # it was built on -- a caller may have swapped modelcp.netG for another copy in between)
    if cached is not None and cached[0] == sig and prev == (modelcp.netG, est_modelcp.netE) and hasattr(cached[1], 'reset'):
        inner = cached[1]
        inner.reset()
    else:
        inner = make_inner_optimizer(opt, modelcp.netG, est_modelcp.netE)
        modelcp._inner_opt = (sig, inner)
    est_model_fixed.feed_data(val_data)
    est_model_fixed.test()
    slr_fixed = est_model_fixed.fake_L
    target = lqs[:, center]
    losses = []
    for _ in range(steps):
        if not opt['train']['use_real']:
            est_modelcp.feed_data(val_data)
            est_modelcp.forward_without_optim()
            slr = est_modelcp.fake_L
        else:
            slr = val_data['SuperLQs']
        inner.zero_grad()
        g_in = backbone_input(opt, slr)                         # TOF: bicubic x scale (test_dynavsr.py:245-250)
        if m['use_patch']:                                      # test_dynavsr.py:255-260
            p_lq, p_gt = crop(g_in, target, m['num_patch'], m['patch_size'], region)
            modelcp.feed_data({'LQs': p_lq, 'GT': p_gt})
        else:
            modelcp.feed_data({'LQs': g_in, 'GT': target})
        loss = modelcp.calculate_loss() if region is None or m['use_patch'] else modelcp.calculate_loss(region=region)
        if region is not None:
            sh, sw = slr_region(region, opt['scale'])
            if slr.is_cuda and loss.is_cuda:
                loss = hipops.inner_loss_region(loss, slr, slr_fixed, (sh, sw), slr_weight)
            else:
                loss = loss + slr_weight * F.l1_loss(slr.to(slr_fixed.device)[..., :sh, :sw], slr_fixed[..., :sh, :sw])
        elif slr.is_cuda and loss.is_cuda:     # one native reduction for the L1 tail (hipops.inner_loss)
            loss = hipops.inner_loss(loss, slr, slr_fixed, slr_weight)
        else:
            loss = loss + slr_weight * F.l1_loss(slr.to(slr_fixed.device), slr_fixed)
        loss.backward()
        inner.step()
        losses.append(loss.detach())
    if not final_test:      # adapt_video runs the adapted forward itself (on another stream)
        return {'sr': None, 'losses': losses, 'slr': slr.detach()}
    modelcp.feed_data({'LQs': backbone_input(opt, lqs)}, need_GT=False)
    modelcp.test()
    return {'sr': modelcp.fake_H, 'losses': losses, 'slr': slr.detach()}


def _meta_batchable(opt, model, est_model, inner):
    m = opt['train']['maml']
    from .models.loss import CharbonnierLoss
    return (inner == 'reference' and not m['use_patch'] and not opt['train']['use_real']
            and hasattr(model.netG, 'forward_stacked') and hasattr(est_model.netE, 'forward_stacked')
            and isinstance(model.cri_pix, CharbonnierLoss) and isinstance(est_model.MyLoss, torch.nn.L1Loss)
            and next(model.netG.parameters()).is_cuda)


def _meta_train_step_batched(opt, model, est_model, train_data, optimizer, group, force_collective):
    """inner='reference' with all B tasks as ONE batch.  In the driver as shipped (quirk Q1) every loss of
    every task is evaluated at the SAME meta-parameters and every gradient lands in the same `.grad`:
        d theta = sum_b [ steps * grad l_train_b + grad l_q_b / B ],   d phi = sum_b [ steps * grad l_train_b + grad l_e_b / (10 B) ]
    (the `steps` inner iterations of a task repeat the same evaluation: the inner optimiser steps nothing).  So the
    estimator runs once on the B clips -- its output serves the inner loss AND loss_e, which the loop computes twice --,
    the backbone once on the B SLR clips and once on the B LR clips, with per-task losses (each task's own mean) summed
    with those weights; one backward.  Same numbers as the task loop (train_dynavsr.py:300-426), B-times fatter launches."""
    from . import dist as D
    m = opt['train']['maml']
    steps = m['adapt_iter']
    lqs, slq, gt = train_data['LQs'], train_data['SuperLQs'], train_data['GT']
    B, center = lqs.size(0), lqs.size(1) // 2
    optimizer.zero_grad()
    est_model.feed_data({'LQs': lqs, 'SuperLQs': slq})
    est_model.forward_without_optim()
    slr = est_model.fake_L                                                   # [B,N,3,h,w], graph into netE
    model.feed_data({'LQs': backbone_input(opt, slr), 'GT': lqs[:, center]})
    model.fake_H = model.netG(model.var_L)
    l_pix = model.l_pix_w * hipops.charbonnier_per_sample(model.fake_H, model.real_H, model.cri_pix.eps)   # [B]
    l1 = hipops.inner_loss_per_sample(torch.zeros_like(l_pix), slr, slq.to(slr.device), 1.0)                 # [B] = loss_e
    l_train = l_pix + l1                                                     # :393, per task
    sr_q = model.netG(backbone_input(opt, lqs))                              # meta test at the same weights (:403)
    l_q = model.l_pix_w * hipops.charbonnier_per_sample(sr_q, gt[:, center], model.cri_pix.eps)
    total = float(steps) * l_train.sum() + l_q.sum() / B + l1.sum() / (B * 10)
    total.backward()
    if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
        D.allreduce_meta_gradients([model.netG, est_model.netE], average=True, group=group, force=force_collective)
    optimizer.step()
    lt, le = l_train.detach(), l1.detach()
    return {'loss_q': float(l_q.detach().sum()) / B, 'loss_train': [lt[b] for b in range(B) for _ in range(steps)],
            'loss_e': [le[b] for b in range(B)], 'batched': True}


def _meta_train_step_copies_batched(opt, model, est_model, modelcp, est_modelcp, train_data, optimizer, group,
                                    force_collective):
    """inner='copies' (first-order MAML, the semantics of the reference's validation / test loops) with all B tasks as
    batches: the B copies adapt together (FrameBatch: first step on the shared weights, later steps on per-task weight
    sets), loss_q and loss_e are taken at the ADAPTED weights of every task in one forward each (per-task weight sets),
    and the meta-gradient is the sum over the task slices of their first-order gradients."""
    from . import dist as D
    m = opt['train']['maml']
    lqs, slq, gt = train_data['LQs'], train_data['SuperLQs'], train_data['GT']
    B, center = lqs.size(0), lqs.size(1) // 2
    optimizer.zero_grad()
    fb = getattr(modelcp, '_meta_batch', None)
    if fb is None or fb.k != B or fb.sig != FrameBatch.signature(opt, model.netG, est_model.netE):
        fb = modelcp._meta_batch = FrameBatch(opt, model.netG, est_model.netE, B)
    losses, _ = fb.adapt(model, est_model, None, lqs, slr_weight=1.0, steps=m['adapt_iter'], slr_ref=slq.to(lqs.device))
    fb.inner.zero_grad()
    sr_q = model.netG.forward_stacked(backbone_input(opt, lqs), fb.g_stack, per_slice=True)
    l_q = model.l_pix_w * hipops.charbonnier_per_sample(sr_q, gt[:, center], model.cri_pix.eps)
    est_model.feed_data({'LQs': lqs, 'SuperLQs': slq})
    y = est_model.netE.forward_stacked(est_model.var_H, fb.e_stack, per_slice=True)
    if est_model.mode != 'image':
        slr = y.transpose(1, 2)
    else:
        b, t, c = lqs.shape[:3]
        slr = y.reshape(b, t, c, y.shape[-2], y.shape[-1])
    l_e = hipops.inner_loss_per_sample(torch.zeros_like(l_q), slr, slq.to(slr.device), 1.0)
    (l_q.sum() / B + l_e.sum() / (B * 10)).backward()
    for p, s_ in zip(model.netG.ordered_parameters(), fb.g_stack):       # :414-415 `param.grad += grads[j]` over the tasks
        p.grad = s_.grad.sum(0)
    for p, s_ in zip(est_model.netE.ordered_parameters(), fb.e_stack):
        p.grad = s_.grad.sum(0)
    modelcp.netG, est_modelcp.netE = fb.netG[B - 1], fb.netE[B - 1]     # the last task's adapted copies, like the loop leaves them
    if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
        D.allreduce_meta_gradients([model.netG, est_model.netE], average=True, group=group, force=force_collective)
    optimizer.step()
    return {'loss_q': float(l_q.detach().sum()) / B, 'loss_train': [l_[b] for b in range(B) for l_ in losses],
            'loss_e': [l_e.detach()[b] for b in range(B)], 'batched': True}


def meta_train_step(opt, model, est_model, modelcp, est_modelcp, train_data, optimizer, inner='reference',
                    group=None, force_collective=False, batched=True):
    """One outer (meta) iteration of the DynaVSR training driver, codes/train_dynavsr.py:265-438, over the
    wrapper API: the tasks of the batch are looped one clip at a time (:300), every task contributes its
    meta-gradient to ``model.netG`` / ``est_model.netE``'s ``.grad``, and the meta optimiser steps once (:438).

    train_data: {'LQs': [B,N,3,h,w], 'SuperLQs': [B,N,3,h/s,w/s], 'GT': [B,N,3,s*h,s*w]} on the GPU.

    inner='reference' (default) reproduces the driver as shipped, quirk Q1 of SURVEY 8a included: the inner losses
    are computed with ``model`` / ``est_model`` (:360-385) while the inner optimiser holds the parameters of the
    deep copies (:326-351), so its step is a no-op and ``loss_train.backward()`` (:397) accumulates straight into
    the meta-gradient; loss_q (:403) and loss_e (:418) are evaluated at the un-adapted weights:
        dθ = Σ_tasks [ Σ_k ∇θ loss_train + ∇θ loss_q / B ],   dφ = Σ_tasks [ Σ_k ∇φ loss_train + ∇φ loss_e / (10 B) ]
    inner='copies' is the first-order MAML the validation / test loops implement (:660-677, test_dynavsr.py:260-277):
    the copies are adapted for adapt_iter steps and loss_q / loss_e are evaluated with the ADAPTED weights, their
    gradients added to the meta-parameters' ``.grad``.

    Multi-GPU: each rank runs this on its shard of the tasks; with ``group`` given (or a default
    process group initialised) the accumulated gradients are all-reduced ONCE (mean over ranks) before the meta
    step -- the reference instead lets DDP hooks fire on every inner backward and leaves loss_q un-reduced; at
    world_size 1 the two coincide.  Returns {'loss_q': Σ loss_q / B, 'loss_train': [...], 'loss_e': [...]}.

    batched (default): in 'reference' mode all tasks are evaluated at the same weights, so they run as ONE batch
    (_meta_train_step_batched: same numbers, B-times fatter launches, the estimator's forward shared between the inner
    loss and loss_e); batched=False keeps the task loop."""
    if batched and _meta_batchable(opt, model, est_model, inner):
        return _meta_train_step_batched(opt, model, est_model, train_data, optimizer, group, force_collective)
    m_ = opt['train']['maml']
    if (batched and inner == 'copies' and _meta_batchable(opt, model, est_model, 'reference') and FrameBatch.supported(opt, model, est_model)
            and (m_['lr_alpha_est'] is None or m_['lr_alpha_est'] == m_['lr_alpha'])):
        return _meta_train_step_copies_batched(opt, model, est_model, modelcp, est_modelcp, train_data, optimizer, group,
                                               force_collective)
    from . import dist as D
    m = opt['train']['maml']
    steps = m['adapt_iter']
    lqs_all = train_data['LQs']
    B, center = lqs_all.size(0), lqs_all.size(1) // 2
    use_real = bool(opt['train']['use_real'])
    optimizer.zero_grad()
    g_params = [p for p in model.netG.parameters()]
    e_params = [p for p in est_model.netE.parameters()]

    def add_grads(params, grads):
        for p, g in zip(params, grads):
            p.grad = g if p.grad is None else p.grad + g       # train_dynavsr.py:414-415 `param.grad += grads[j]`

    total_q, log_train, log_e = 0.0, [], []
    for b in range(B):
        task = {k: train_data[k][b:b + 1] for k in ('LQs', 'GT', 'SuperLQs')}
        lr_target = task['LQs'][:, center]                      # meta-train target: the LR centre frame (:288)
        hr_target = task['GT'][:, center]                       # meta-test target (:290)
        modelcp.netG, est_modelcp.netE = _fresh_copy(modelcp.netG, model.netG), _fresh_copy(est_modelcp.netE, est_model.netE)
        inner_model, inner_est = (model, est_model) if inner == 'reference' else (modelcp, est_modelcp)
        groups = [{'params': [p for p in modelcp.netG.parameters() if p.requires_grad], 'lr': m['lr_alpha']},
                  {'params': [p for p in est_modelcp.netE.parameters() if p.requires_grad],
                   'lr': m['lr_alpha_est'] if m['lr_alpha_est'] is not None else m['lr_alpha']}]
        if m['optimizer'] == 'Adam':
            inner_opt = torch.optim.Adam(groups, lr=m['lr_alpha'], betas=(m['beta1'], m['beta2']))
        elif m['optimizer'] == 'SGD':
            inner_opt = torch.optim.SGD(groups, lr=m['lr_alpha'])
        else:
            raise NotImplementedError()
        for _ in range(steps):
            inner_opt.zero_grad()
            if not use_real:
                inner_est.feed_data(task)
                inner_est.forward_without_optim()
                slr = inner_est.fake_L
            else:
                slr = task['SuperLQs']
            g_in = backbone_input(opt, slr)                     # TOF: bicubic x scale (train_dynavsr.py:368-374)
            if m['use_patch']:                                  # train_dynavsr.py:377-382
                p_lq, p_gt = crop(g_in, lr_target, m['num_patch'], m['patch_size'])
                inner_model.feed_data({'LQs': p_lq, 'GT': p_gt})
            else:
                inner_model.feed_data({'LQs': g_in, 'GT': lr_target})
            loss_train = inner_model.calculate_loss()
            loss_train = loss_train + F.l1_loss(slr, task['SuperLQs'].to(slr.device))      # :393
            loss_train.backward()
            inner_opt.step()
            log_train.append(loss_train.detach())
        # meta test: loss_q at the weights `model` holds ('reference') or at the adapted copy ('copies')
        q_model, q_est = (model, est_model) if inner == 'reference' else (modelcp, est_modelcp)
        q_model.feed_data({'LQs': backbone_input(opt, task['LQs']), 'GT': hr_target})   # (:314-320 for TOF)
        loss_q = q_model.calculate_loss()
        add_grads(g_params, torch.autograd.grad(loss_q / B, list(q_model.netG.parameters())))
        q_est.feed_data(task)
        q_est.forward_without_optim()
        loss_e = est_model.MyLoss(q_est.fake_L, q_est.real_L)
        add_grads(e_params, torch.autograd.grad(loss_e / (B * 10), list(q_est.netE.parameters())))
        total_q += float(loss_q.detach()) / B
        log_e.append(loss_e.detach())
    if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
        D.allreduce_meta_gradients([model.netG, est_model.netE], average=True, group=group, force=force_collective)
    optimizer.step()
    return {'loss_q': total_q, 'loss_train': log_train, 'loss_e': log_e}


def validate_video(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, clips, gts, rank=0, world=1, group=None,
                   frames_per_batch=1, overlap=True):
    """The validation loop of train_dynavsr.py:500-728 / the test driver's per-frame evaluation: this rank adapts and
    super-resolves the frames range(rank, len(clips), world) (adapt_video), PSNR of the un-adapted ('start') and of the
    adapted ('final') output against ``gts[i]`` [3,sH,sW] with the reference's uint8 definition, computed on the device
    (utils.util.frame_metrics, no per-frame host sync); the two vectors are reduced to rank 0 (dist.validate_sharded).
    Returns {'psnr_start', 'psnr_final'} as float64 tensors of length len(clips) (complete on rank 0; NaN where this rank
    holds no result; +inf for an exact match, as util.calculate_psnr), 'evaluated' (bool mask) and 'frames'."""
    from . import dist as D
    from .utils import util
    dev = next(model.netG.parameters()).device

    def run(indices):
        mine = [clips[i] for i in indices]
        for i, (base, r) in zip(indices, adapt_video(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, mine,
                                                     overlap=overlap, frames_per_batch=frames_per_batch)):
            gt = gts[i].to(dev)
            yield (util.frame_metrics(base[0], gt, need_img=None)[0], util.frame_metrics(r['sr'][0], gt, need_img=None)[0], 1.0)
    mse_s, mse_f, seen = D.validate_sharded(len(clips), run, rank, world, group, dev, n_metrics=3)
    # A separate 'evaluated' vector travels with the two MSE vectors (all zero-initialised, summed to rank 0): an exact match
    # (mse == 0) is +inf dB like util.calculate_psnr, an entry this rank does not hold (other ranks' frames off rank 0) is NaN.
    seen = seen > 0
    inf, nan = float('inf'), float('nan')

    def psnr(m):
        v = torch.where(m > 0, 20 * torch.log10(255.0 / torch.sqrt(m.clamp_min(1e-300))), torch.full_like(m, inf))
        return torch.where(seen, v, torch.full_like(m, nan))
    return {'psnr_start': psnr(mse_s), 'psnr_final': psnr(mse_f), 'evaluated': seen,
            'frames': D.shard_indices(len(clips), rank, world)}


class FrameBatch:
    """K frames adapted as ONE batch (north_star: the inner MAML step; test_dynavsr.py:208-277 with adapt_iter = 1).

    The reference deep-copies netG / netE for every frame and takes one optimiser step on the copy.  All K copies start
    from the same un-adapted weights, so the K forward + backward passes differ only in their data: they run as one
    batch of K clips through the tapes (launches K times fatter than the 44x80 grids of a single SLR clip), with
    PER-CLIP parameter gradients (dvsr_edvr_plan_create_grouped).  The K private copies are the slices of stacked
    [K, *shape] tensors; ONE elementwise optimiser step over the stacks is the K independent inner updates.  The
    per-frame modules `netG[k]` / `netE[k]` alias the slices (state-dict compatible with the reference's copies)."""

    def __init__(self, opt, netG, netE, k):
        self.k = k
        m = opt['train']['maml']
        self.scale = opt['scale']
        self.sig = self.signature(opt, netG, netE)
        with torch.no_grad():
            self.g_stack = [torch.empty((k,) + tuple(p.shape), dtype=torch.float32, device=p.device).requires_grad_()
                            for p in netG.ordered_parameters()]
            self.e_stack = [torch.empty((k,) + tuple(p.shape), dtype=torch.float32, device=p.device).requires_grad_()
                            for p in netE.ordered_parameters()]
        params = self.g_stack + self.e_stack
        if m['optimizer'] == 'Adam':
            self.inner = optim.Adam(params, lr=m['lr_alpha'], betas=(m['beta1'], m['beta2']))
        elif m['optimizer'] == 'SGD':
            self.inner = optim.SGD(params, lr=m['lr_alpha'])
        else:
            raise NotImplementedError()
        self.netG, self.netE = [], []
        for i in range(k):                               # frame i's networks: parameters are slice i of the stacks
            g, e = deepcopy(netG), deepcopy(netE)
            for p, s_ in zip(g.ordered_parameters(), self.g_stack):
                p.data = s_.data[i]
            for p, s_ in zip(e.ordered_parameters(), self.e_stack):
                p.data = s_.data[i]
            self.netG.append(g); self.netE.append(e)
        self.last_use = None                             # event: the last forward that read these weights
        self._rep = None                                 # cached pointer arrays of refresh()

    @staticmethod
    def signature(opt, netG, netE):
        m = opt['train']['maml']
        return (m['optimizer'], m['lr_alpha'], m.get('beta1'), m.get('beta2'), type(netG), type(netE),
                tuple(tuple(p.shape) for p in netG.ordered_parameters()), tuple(tuple(p.shape) for p in netE.ordered_parameters()),
                str(next(netG.parameters()).device))

    @staticmethod
    def supported(opt, model, est_model):
        """What the batched step covers; everything else takes the per-frame loop."""
        m = opt['train']['maml']
        from .models.loss import CharbonnierLoss
        ok = (m['adapt_iter'] >= 1 and not m['use_patch'] and not opt['train']['use_real']
              and hasattr(model.netG, 'forward_stacked') and hasattr(est_model.netE, 'forward_stacked')
              and isinstance(model.cri_pix, CharbonnierLoss) and next(model.netG.parameters()).is_cuda
              and not list(model.netG.buffers()) and not list(est_model.netE.buffers()))
        if not ok:
            return False
        # what the per-sample weight sets of the native tapes need (dvsr_edvr_plan_create_ex: whole 8-channel deformable
        # groups; the fused DCN backward: whole 64-cout blocks; no DVSR_CONV_V1 A/B kernel) -- anything else would raise
        # DVSR_ERR_UNSUPPORTED in the middle of a batch instead of taking the per-frame loop
        import os
        nf, groups = int(model.netG.nf), int(model.netG.groups)
        return (nf % 64 == 0 and groups > 0 and nf % groups == 0 and (nf // groups) % 8 == 0
                and os.environ.get("DVSR_CONV_V1", "0") in ("", "0"))

    def refresh(self, netG, netE):
        """Every slice = the un-adapted weights (the per-frame deepcopy), fresh optimiser state."""
        import ctypes
        from . import _lib as L
        src = netG.ordered_parameters() + netE.ordered_parameters()
        n = len(src)
        if self._rep is None:
            dst = self.g_stack + self.e_stack
            self._rep = ((ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(*[L.ptr(d) for d in dst]),
                         (ctypes.c_longlong * n)(*[p.numel() for p in src]))
        for i, p in enumerate(src):            # (the meta-parameters may have been re-pointed: `param.data = ...`)
            self._rep[0][i] = L.ptr(p.detach() if p.is_contiguous() else p.detach().contiguous())
        L.check(L.lib().dvsr_replicate_tensors(self._rep[0], self._rep[1], self._rep[2], n, self.k, L.stream()),
                "dvsr_replicate_tensors")
        for s_ in self.g_stack + self.e_stack:
            s_.grad = None
        self.inner.reset()
        for g, e in zip(self.netG, self.netE):       # (train() walks ~150 holder modules: only when the mode differs)
            if g.training != netG.training:
                g.train(netG.training)
            if e.training != netE.training:
                e.train(netE.training)

    def adapt(self, model, est_model, est_model_fixed, lqs, slr_weight=10.0, steps=1, slr_ref=None, region=None):
        """lqs [K,N,3,H,W] -> (per-step list of per-frame losses [K], SLR clips [K,N,3,h,w]); afterwards slice k holds
        frame k's adapted weights.  Same statements as adapt_frame's step loop, on the batch.  The SLR term's reference is
        the frozen estimator's output (test time, test_dynavsr.py:264-274) or, with ``slr_ref``, a given clip (meta-training:
        the dataset's SuperLQs with weight 1, train_dynavsr.py:393).  region = (h, w): the clips' valid LR size, as in
        adapt_frame (the per-frame region losses of hipops); None, or the whole clip, is every call of before."""
        assert lqs.size(0) == self.k
        if region is not None:
            region = hipops.check_region(lqs.shape, region, "region")
            if region == (int(lqs.shape[-2]), int(lqs.shape[-1])):
                region = None
        self.refresh(model.netG, est_model.netE)
        center = lqs.size(1) // 2
        if slr_ref is None:
            est_model_fixed.feed_data({'LQs': lqs})
            est_model_fixed.test()
            slr_fixed = est_model_fixed.fake_L
        else:
            slr_fixed = slr_ref
        est_model.feed_data({'LQs': lqs})                 # the wrapper's own layout handling ('video' / 'image' mode)
        losses = []
        for step in range(steps):
            # step 0: every slice still equals the un-adapted network -> one weight set for the batch (one pack);
            # later steps: the copies have diverged -> clip k runs on slice k (dvsr_*_plan_create_ex, weight_sets = K)
            diverged = step > 0
            y = est_model.netE.forward_stacked(est_model.var_H, self.e_stack, per_slice=diverged)
            if est_model.mode != 'image':
                slr = y.transpose(1, 2)
            else:
                b, t, c = lqs.shape[:3]
                slr = y.reshape(b, t, c, y.shape[-2], y.shape[-1])
            sr = model.netG.forward_stacked(slr, self.g_stack, per_slice=diverged)
            if region is None:
                l_pix = model.l_pix_w * hipops.charbonnier_per_sample(sr, lqs[:, center], model.cri_pix.eps)
                loss = hipops.inner_loss_per_sample(l_pix, slr, slr_fixed, slr_weight)
            else:
                l_pix = model.l_pix_w * hipops.charbonnier_region(sr, lqs[:, center], region, model.cri_pix.eps, per_sample=True)
                loss = hipops.inner_loss_region(l_pix, slr, slr_fixed, slr_region(region, self.scale), slr_weight,
                                                per_sample=True)
            self.inner.zero_grad()
            loss.sum().backward()                          # d loss_k / d (slice k) only: the losses share no weights
            self.inner.step()
            losses.append(loss.detach())
        return losses, slr.detach()

    def super_resolve(self, lqs):
        """The adapted outputs of the K frames (test_dynavsr.py:279-283) as ONE forward: clip k on slice k."""
        with torch.no_grad():
            return self.netG[0].forward_stacked(lqs, [s_.detach() for s_ in self.g_stack], per_slice=True)


_EXTRA_STREAMS = {}


def _side_streams(lqs_device):
    """The side stream of the full-size forwards, created once per device: the caching allocator keeps one block pool per
    stream, and the 3 GB workspaces must come back from the pool, not from hipMalloc, on every call.  ONE stream carries
    both the next clip's baseline forward and the current clip's adapted forward: on two streams they run concurrently
    with each other as well whenever ROCm gives them separate hardware queues (GPU_MAX_HW_QUEUES >= 5), and three
    full-size tapes side by side take 32.5 ms per frame against 27.3 sequential and 23.3 with one stream (which is what
    two streams measured only while they happened to share a queue).  (The first of super_resolve_video's extra streams.)"""
    a = _clip_streams(lqs_device, 2)[1]
    return (a, a)


def _clip_streams(device, n):
    """The caller's current stream + n - 1 further HIP streams of the device.  The further ones are created once and shared
    with adapt_video's forward stream (_side_streams): one block pool of the caching allocator and one launch plan +
    workspace per stream must be found again on the next call -- and every extra stream a process has used takes part in
    ROCm's stream -> hardware-queue assignment, which the legs with a weight-gradient side stream are sensitive to (DESIGN
    3.1c; with two private streams here the per-frame pipeline that ran afterwards measured 61 instead of 71 frames/s)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    have = _EXTRA_STREAMS.setdefault(key, [])
    while len(have) < n - 1:
        have.append(torch.cuda.Stream(device=key))
    return [torch.cuda.current_stream(key)] + have[:n - 1]


def _check_flip_test(flip_test, who):
    if not isinstance(flip_test, bool):
        raise ValueError("%s: flip_test=%r must be a bool" % (who, flip_test))


def _flip_test_forward(opt, net, lq):
    """flipx4_forward of the reference (utils/util.py:232-254) on one clip [B,N,3,H,W], on the current stream: the forward
    on the clip and on its three mirror images (frames.flip), then the un-flips and the mean in one launch (frames.flip_mean)."""
    from . import frames as fio
    if lq.dtype != torch.float32 or not lq.is_contiguous() or lq.data_ptr() % 16:
        lq = lq.float().clone(memory_format=torch.contiguous_format)
    ys = [net(backbone_input(opt, lq if v == 0 else fio.flip(lq, v))) for v in range(4)]
    return fio.flip_mean(*[y if y.is_contiguous() else y.contiguous() for y in ys])


def super_resolve_video(opt, net, clips, in_flight=2, flip_test=False):
    """The un-adapted forward of test_dynavsr.py:200-204 (`model.feed_data(val_data, need_GT=False); model.test()`) over a
    stream of clips, as a generator: yields the SR frame [B, 3, sH, sW] of every clip [B, N, 3, H, W], in order.

    `in_flight` clips are on the GPU at a time, one HIP stream each (round robin: the caller's stream and in_flight - 1
    further ones).  A single EDVR-M forward at 180x320 is 85 dependent launches of 1125-workgroup grids on 256 CUs -- 4.4
    rounds of workgroups each, the last one 40 % full, and 5-6 us of idle GPU between two launches -- and a second queue
    fills both: 161.9 -> 187.9 frames/s with two clips in flight, 189.2 with three (tools/fwd_concurrent.py; one forward
    over a batch of 8 clips: 180.4).  Every clip runs the launches it would run alone (its own plan and workspace, keyed
    by the stream) except the weight packing, which only the first clip on a stream does (the workspace and the packs in it
    are kept for the video; an in-place update of the weights between clips re-packs), so the outputs are bit-identical to
    `net(clip)`.  A yielded frame stays valid until the generator is
    advanced `in_flight` times; clips and results are ordered against the caller's current stream.

    flip_test=True: the reference's x4 self-ensemble (`flip_test` of test_Vid4_REDS4_with_GT.py, util.flipx4_forward) -- per
    clip four forwards, on the clip and on frames.flip of it in W, in H and in both, and one frames.flip_mean that un-flips
    and averages them in the reference's order, all on the clip's stream; the clip's and the output's width must be
    multiples of 4.  False takes exactly the calls above.  (The x8 ensemble with transposes is not provided.)"""
    _check_flip_test(flip_test, "super_resolve_video")
    main = None
    streams = None
    pending = []
    # one workspace per (plan, stream) for the whole video, and with it the packed weights: the network is the same for every
    # clip, so only the first forward on a stream packs (engine.FrozenWeights; keyed on the parameters' version counters)
    frozen = engine.FrozenWeights()
    was_training = net.training
    net.eval()
    try:
        for i, c in enumerate(clips):
            lq = c['LQs'] if isinstance(c, dict) else c
            if not lq.is_cuda:
                lq = lq.cuda()
            if streams is None:
                # (the caller's stream ON THE CLIPS' DEVICE -- not the current device's, which may be another one)
                main = torch.cuda.current_stream(lq.device)
                streams = _clip_streams(lq.device, max(1, int(in_flight)))
            if len(pending) == len(streams):         # the oldest clip ran on the stream this one is about to take
                sr, ev = pending.pop(0)
                main.wait_event(ev)
                sr.record_stream(main)
                yield sr
            s = streams[i % len(streams)]
            if s != main:
                s.wait_stream(main)                  # the clip (and the weights) were produced on the caller's stream
            with torch.cuda.stream(s), torch.no_grad(), frozen:
                sr = _flip_test_forward(opt, net, lq) if flip_test else net(backbone_input(opt, lq))
                ev = torch.cuda.Event()
                ev.record(s)
            if s != main:
                lq.record_stream(s)
            pending.append((sr, ev))
        while pending:
            sr, ev = pending.pop(0)
            main.wait_event(ev)
            sr.record_stream(main)
            yield sr
    finally:
        # a generator closed early leaves forwards running on the side streams: whatever the caller does next on its stream
        # (an inner step updates the weights they read) must come behind them
        for sr, ev in pending:
            main.wait_event(ev)
            sr.record_stream(main)
        net.train(was_training)


def adapt_video(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, clips, overlap=True, frames_per_batch=1,
                region=None, baseline=True):
    """The frame loop of test_dynavsr.py:197-283 as a generator: for every clip {'LQs': [1,N,3,H,W]} yields
    (baseline SR, adapt_frame's result dict with the adapted 'sr').

    frames_per_batch = K > 1: the inner steps of K consecutive frames run as ONE batch with per-frame parameter gradients
    (FrameBatch; needs adapt_iter = 1, the value of every shipped YAML, Charbonnier pixel loss, no use_patch / use_real --
    otherwise the per-frame loop below is taken).  Per-frame results are those of the per-frame loop (same kernels on the
    same inputs; launch geometry and atomic summation order differ at the 1e-6 level).

    Per clip the loop is baseline forward (un-adapted network, :200-204) -> inner steps on copies -> adapted
    forward.  The two full-size forwards do not depend on the NEXT clip's adaptation, and the inner step works on a
    16x smaller grid whose launches fill a fraction of the 256 CUs -- so with ``overlap`` the next clip's baseline
    and the current clip's adapted forward run on a further HIP stream underneath the following adaptation
    (two alternating sets of copies, so a forward never reads weights that are being refreshed).  Results are
    those of the sequential loop (same kernels, same inputs).  A yielded result stays valid until the generator
    is advanced twice (frames_per_batch = K > 1: until it is advanced 2 K times).

    region = (h, w): every clip's valid LR size (adapt_frame / FrameBatch.adapt); None, or the whole clip, is every call of
    before.  baseline=False skips the un-adapted forward, which only reports and is a third of a frame's device
    time: the generator then yields (None, result).  True is every call of before."""
    if frames_per_batch > 1 and FrameBatch.supported(opt, model, est_model):
        yield from _adapt_video_batched(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, clips, overlap,
                                        frames_per_batch, region, baseline)
        return
    clips = iter(clips)
    cur = next(clips, None)
    if cur is None:
        return
    main = torch.cuda.current_stream()
    if not overlap:
        while cur is not None:
            lqs = cur['LQs'] if cur['LQs'].is_cuda else cur['LQs'].cuda()
            if baseline:
                model.feed_data({'LQs': backbone_input(opt, lqs)}, need_GT=False)
                model.test()
            yield (model.fake_H if baseline else None,
                   adapt_frame(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, cur, region=region))
            cur = next(clips, None)
        return
    s_base, s_test = _side_streams(lqs_device=cur['LQs'].device if cur['LQs'].is_cuda else torch.device('cuda'))
    sets = [[modelcp.netG, est_modelcp.netE, getattr(modelcp, '_inner_opt', None), None],
            [None, None, None, None]]                # [netG copy, netE copy, cached inner optimiser, last-use event]

    def forward_on(stream, net, lqs):
        stream.wait_stream(main)                     # weights / clip were produced on the main stream
        with torch.cuda.stream(stream), torch.no_grad():
            was_training = net.training
            net.eval()
            sr = net(backbone_input(opt, lqs))
            net.train(was_training)
            ev = torch.cuda.Event()
            ev.record(stream)
        # the clip was allocated on the main stream and is read here until the END of the tape (base_up reads the
        # centre frame last): tell the caching allocator, or a transient clip (a `.cuda()` copy of a CPU clip, a
        # generator's temporary) is handed out again on the main stream while this forward is still in flight
        lqs.record_stream(stream)
        return sr, ev

    def on_gpu(data):
        return data['LQs'] if data['LQs'].is_cuda else data['LQs'].cuda()

    def hand_out(out):
        (p0, pe0), (p1, pe1), pr = out
        if p0 is not None:
            main.wait_event(pe0)
            p0.record_stream(main)
        main.wait_event(pe1)
        p1.record_stream(main)
        pr['sr'] = p1
        return p0, pr

    pending, i, prev_out = (forward_on(s_base, model.netG, on_gpu(cur)) if baseline else (None, None)), 0, None
    while cur is not None:
        nxt = next(clips, None)
        lqs = on_gpu(cur)
        sr0, ev0 = pending
        if nxt is not None and baseline:
            pending = forward_on(s_base, model.netG, on_gpu(nxt))   # enqueued first: runs underneath the adaptation
        st = sets[i & 1]
        if st[3] is not None:
            main.wait_event(st[3])                   # this set's previous adapted forward has read its weights
        modelcp.netG, est_modelcp.netE, modelcp._inner_opt = st[0], st[1], st[2]
        r = adapt_frame(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, {'LQs': lqs}, final_test=False,
                        region=region)
        st[0], st[1], st[2] = modelcp.netG, est_modelcp.netE, getattr(modelcp, '_inner_opt', None)
        sr1, ev1 = forward_on(s_test, modelcp.netG, lqs)
        st[3] = ev1
        if prev_out is not None:                     # hand out clip i-1 now that clip i's work is enqueued
            yield hand_out(prev_out)
        prev_out = ((sr0, ev0), (sr1, ev1), r)
        cur, i = nxt, i + 1
    yield hand_out(prev_out)


def _adapt_video_batched(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, clips, overlap, K, region=None,
                         baseline=True):
    """adapt_video with the inner steps of K consecutive frames as one batch.  With ``overlap`` the 2K full-size forwards
    of a chunk (un-adapted baselines, adapted outputs) run on the side stream underneath the NEXT chunk's batched inner
    step; two alternating FrameBatch sets, so a forward never reads weights that are being refreshed."""
    it = iter(clips)

    def take(first=None):
        chunk = [first] if first is not None else []
        if len(chunk) == K:
            return chunk, None
        for c in it:
            lq = c['LQs'] if c['LQs'].is_cuda else c['LQs'].cuda()
            assert lq.size(0) == 1
            if chunk and lq.shape != chunk[0].shape:       # a new sequence size: close the chunk, keep the clip
                return chunk, lq
            chunk.append(lq)
            if len(chunk) == K:
                break
        return chunk, None

    main = torch.cuda.current_stream()
    side = None
    cache = getattr(modelcp, '_frame_batches', None)
    if cache is None:
        cache = modelcp._frame_batches = {}

    def batch_for(parity, k):
        fb = cache.get((parity, k))
        if fb is None or fb.sig != FrameBatch.signature(opt, model.netG, est_model.netE):
            fb = cache[(parity, k)] = FrameBatch(opt, model.netG, est_model.netE, k)
        return fb

    def run(net, lq):
        if isinstance(net, FrameBatch):
            return net.super_resolve(lq)
        was = net.training
        net.eval()
        sr = net(backbone_input(opt, lq))
        net.train(was)
        return sr

    def forward_on(net, lq):
        if side is None:
            with torch.no_grad():
                return run(net, lq), None
        side.wait_stream(main)
        with torch.cuda.stream(side), torch.no_grad():
            sr = run(net, lq)
            ev = torch.cuda.Event()
            ev.record(side)
        lq.record_stream(side)
        return sr, ev

    def hand_out(out):
        base, adapted, losses, slr, fb = out
        for k_, ((b_sr, b_ev), (a_sr, a_ev)) in enumerate(zip(base, adapted)):
            if a_ev is not None:
                if k_ == 0:
                    if b_ev is not None:
                        main.wait_event(b_ev)
                    main.wait_event(a_ev)
                if b_sr is not None:
                    b_sr.record_stream(main)
                a_sr.record_stream(main)
            modelcp.netG, est_modelcp.netE = fb.netG[k_], fb.netE[k_]     # the frame's adapted copies, like the reference's modelcp
            yield b_sr, {'sr': a_sr, 'losses': [l_[k_] for l_ in losses], 'slr': slr[k_:k_ + 1]}

    chunk, carry = take()
    pending, ci = None, 0
    while chunk:
        if overlap and side is None:
            side = _side_streams(chunk[0].device)[0]
        lqs = torch.cat(chunk) if len(chunk) > 1 else chunk[0]
        # the un-adapted baselines of the chunk share their weights too: ONE forward over the K clips (N = K through the
        # trunk instead of 450 tiles on 256 CUs; the small pyramid levels K times fatter); enqueued first, it runs
        # underneath the adaptation
        b_sr, b_ev = forward_on(model.netG, lqs) if baseline else (None, None)
        base = [(b_sr[k_:k_ + 1] if baseline else None, b_ev) for k_ in range(len(chunk))]
        fb = batch_for(ci & 1, len(chunk))
        if fb.last_use is not None:
            main.wait_event(fb.last_use)                                 # this set's previous adapted forwards are done
        losses, slr = fb.adapt(model, est_model, est_model_fixed, lqs, steps=opt['train']['maml']['adapt_iter'], region=region)
        # the K adapted forwards as ONE forward with per-frame weights (backbone_input: identity for EDVR, the only
        # backbone FrameBatch takes)
        a_sr, a_ev = forward_on(fb, lqs)
        adapted = [(a_sr[k_:k_ + 1], a_ev) for k_ in range(len(chunk))]
        fb.last_use = a_ev
        if pending is not None:
            yield from hand_out(pending)
        pending = (base, adapted, losses, slr, fb)
        chunk, carry = take(carry)          # (a clip of another size that closed this chunk starts the next one)
        ci += 1
    if pending is not None:
        yield from hand_out(pending)


def scene_bounds(T, cuts):
    """The scenes [(a, b), ...] of a video of T frames cut at `cuts`: a strictly increasing sequence of ints in (0, T), k
    meaning that frame k is the first frame of a new scene ([] = one scene).  Anything else is a ValueError."""
    import numbers
    T = int(T)
    if isinstance(cuts, (str, bytes)) or not hasattr(cuts, '__iter__'):
        raise ValueError("cuts=%r: a sequence of frame numbers (or None)" % (cuts,))
    ks = list(cuts)
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise ValueError("cuts: %r is not an int" % (k,))
    ks = [int(k) for k in ks]
    for i, k in enumerate(ks):
        if not 0 < k < T:
            raise ValueError("cuts: %d is outside (0, %d) -- a cut names the first frame of a new scene" % (k, T))
        if i and k <= ks[i - 1]:
            raise ValueError("cuts: %s is not strictly increasing" % (ks,))
    edges = [0] + ks + [T]
    return list(zip(edges[:-1], edges[1:]))


def video_windows(T, nframes, padding='new_info', cuts=None):
    """(windows, scenes): the window (list of nframes frame numbers) of every centre 0 .. T - 1, and the number of scenes.

    cuts=None: one scene, data.util.index_generation(centre, T, nframes, padding); ValueError where a window leaves [0, T).
    Scene mode (any other `cuts`, see scene_bounds): the window of centre c in the scene [a, b) is
    a + index_generation(c - a, b - a, nframes, padding) -- what the reference's datasets give, which read one folder per
    scene -- and a scene too short for `padding` (some window would leave [a, b)) takes 'replicate', which never leaves it,
    for all of its windows.  Nothing is raised for a short scene."""
    from .data.util import index_generation
    T, nframes = int(T), int(nframes)
    if cuts is None:
        windows = [index_generation(c, T, nframes, padding) for c in range(T)]
        for c, win in enumerate(windows):
            if min(win) < 0 or max(win) >= T:
                raise ValueError("stream_schedule: %d frames are too few for windows of %d under padding %r (centre %d would "
                                 "read frames %s)" % (T, nframes, padding, c, win))
        return windows, 1
    scenes = scene_bounds(T, cuts)
    windows = []
    for a, b in scenes:
        wins = [index_generation(c, b - a, nframes, padding) for c in range(b - a)]
        if any(min(win) < 0 or max(win) >= b - a for win in wins):
            wins = [index_generation(c, b - a, nframes, 'replicate') for c in range(b - a)]
        windows += [[a + i for i in win] for win in wins]
    return windows, len(scenes)


def stream_slots(nframes, in_flight, scenes=1):
    """The capacity of the frame cache that stream_schedule assumes (see there)."""
    if scenes > 1 and in_flight > 1:
        return 2 * nframes + in_flight - 2
    return nframes + in_flight - 1


def stream_schedule(T, nframes, padding='new_info', in_flight=2, cuts=None):
    """The frame-cache schedule of super_resolve_frames, as pure Python: for every centre frame 0 .. T - 1 yields
    (centre, frames_to_extract, [(frame, slot), ...], window_slots).

    The window of a centre is data.util.index_generation(centre, T, nframes, padding).  A frame is extracted when a
    window first needs it; frames go in increasing order, each exactly once (a window that needs frame f finds 0 .. f
    extracted), frame f into slot f % slots of a cache of slots = nframes + in_flight - 1.  That capacity is enough for
    the four padding modes: a frame is overwritten nframes + in_flight - 1 frames later, when neither the current window,
    nor the in_flight - 1 before it that may still be running, nor any later one names it (tests/test_stream_schedule.py
    simulates it).  window_slots are the cache slots of the window's frames, in window order.
    T < nframes is accepted only where every window stays inside [0, T); otherwise ValueError, where the reference would
    index past the end of its frame list.

    cuts (None: all of the above, unchanged): scene mode, the windows of video_windows -- no window names a frame of
    another scene, and a short scene raises nothing.  The properties are the same; the capacity is not.  With more than
    one scene the windows that end a scene reach nframes frames back while the first window of the next one reaches
    nframes - 1 frames ahead, and the smallest cache that always works with slot = frame % slots is
        slots = nframes                        for in_flight == 1,
        slots = 2 * nframes + in_flight - 2    otherwise
    (stream_slots; found and held by simulation over nframes 3, 5, 7, in_flight 1 .. 4, the four modes, T <= 29 and cut
    sets of every single cut, a cut at every frame and random ones: tests/test_scene_schedule.py, which also shows that
    one slot fewer fails).  One scene (cuts=[]) keeps nframes + in_flight - 1."""
    T, nframes, in_flight = int(T), int(nframes), int(in_flight)
    if T < 1 or nframes < 1 or in_flight < 1:
        raise ValueError("stream_schedule: T=%d, nframes=%d, in_flight=%d must be positive" % (T, nframes, in_flight))
    windows, scenes = video_windows(T, nframes, padding, cuts)
    slots = stream_slots(nframes, in_flight, scenes)
    done = 0                       # frames 0 .. done - 1 are extracted
    for c, win in enumerate(windows):
        new = list(range(done, max(done, max(win) + 1)))
        done += len(new)
        yield c, new, [(f, f % slots) for f in new], [f % slots for f in win]


def _video_format(frames, layout, who="super_resolve_frames"):
    """(layout, h, w) of a video -- a [T,...] tensor or a list of frames of one kind and size.  No GPU call."""
    from . import frames as fio
    if len(frames) < 1:
        raise ValueError("%s: no frames" % who)
    first = fio.resolve_layout(frames[0], layout)
    if not torch.is_tensor(frames):
        def kind(f):        # a tensor's, or those of the planes of a YCbCr frame
            if torch.is_tensor(f):
                return f.dtype, tuple(f.shape)
            return [kind(p) for p in f] if isinstance(f, (tuple, list)) else type(f).__name__
        for i, f in enumerate(frames):
            if kind(f) != kind(frames[0]):
                raise ValueError("%s: frame %d is %s, frame 0 is %s" % (who, i, kind(f), kind(frames[0])))
            fio.resolve_layout(f, layout)
    return first


MAX_IMAGE_BYTES = 1 << 32     # the conv and DCN kernels address one image of a tensor with 32-bit offsets (csrc/common.h)


def tile_origins(n, tile, overlap):
    """The origins of the tiles of one axis of padded length n (a multiple of 4), in LR pixels: tile a multiple of 4, overlap a
    multiple of 4 with 0 <= overlap <= tile / 2.  tile >= n: [0], one tile of length n.  Otherwise step = tile - overlap and
    the origins are k * step for every k * step < n - tile, then n - tile: every tile has the same size, the last one is anchored
    at the edge, every origin is a multiple of 4 and a position is covered by at most 3 tiles (dvsr_frame_stitch_origins; host
    code)."""
    import ctypes
    from . import _lib as L
    n, tile, overlap = int(n), int(tile), int(overlap)
    count = L.lib().dvsr_frame_stitch_origins(n, tile, overlap, None, 0)
    if count < 1:
        raise ValueError("tile_origins: " + L.lib().dvsr_last_error().decode("utf-8", "replace"))
    arr = (ctypes.c_int * count)()
    L.lib().dvsr_frame_stitch_origins(n, tile, overlap, arr, count)
    return list(arr)


def _check_tile(tile, overlap, budget=None, who="super_resolve_frames"):
    """(tile, overlap) of the tile arguments: tile is None, 'auto' or (th, tw); ValueError for anything else.  No GPU call."""
    import numbers

    def integral(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if not integral(overlap) or overlap < 0 or overlap % 4:
        raise ValueError("%s: tile_overlap=%r must be a multiple of 4, >= 0" % (who, overlap))
    if budget is not None and not (isinstance(tile, str) and tile == 'auto'):
        raise ValueError("%s: tile_budget is the budget of tile='auto', got tile=%r" % (who, tile))
    if budget is not None and (isinstance(budget, bool) or not isinstance(budget, numbers.Real) or not budget > 0):
        raise ValueError("%s: tile_budget=%r must be a positive number of bytes" % (who, budget))
    if tile is None:
        return None, int(overlap)
    if isinstance(tile, str):
        if tile != 'auto':
            raise ValueError("%s: tile=%r (None, 'auto', an int or (th, tw))" % (who, tile))
        return 'auto', int(overlap)
    if integral(tile):
        tile = (tile, tile)
    if not isinstance(tile, (tuple, list)) or len(tile) != 2 or not all(integral(v) for v in tile):
        raise ValueError("%s: tile=%r (None, 'auto', an int or (th, tw))" % (who, tile))
    for v in tile:
        if v % 4 or v < 16 or v < 2 * overlap:
            raise ValueError("%s: tile=%r with tile_overlap=%d: a tile side is a multiple of 4, at least 16 and at least twice the "
                             "overlap" % (who, tuple(tile), overlap))
    return (int(tile[0]), int(tile[1])), int(overlap)


def _tile_parts(net, h, w, tile, overlap, in_flight, scenes=1, flip_test=False, multiple=4):
    """tile_footprint's terms as a dict, 'plan' (a StreamPlan built for the query alone, never run), 'tile' and 'grid' beside
    them."""
    from . import frames as fio
    from .models.archs.EDVR_arch import EDVR
    if not isinstance(net, EDVR):
        raise ValueError("tile_footprint: the footprint comes from an EDVR stream plan's queries; got %s" % type(net).__name__)
    tile, overlap = _check_tile(tile, overlap, who="tile_footprint")
    if tile == 'auto':
        raise ValueError("tile_footprint: tile='auto' is choose_tile's answer, pass it")
    in_flight, scenes, mult = max(1, int(in_flight)), max(1, int(scenes)), int(multiple)
    mult *= 4 // math.gcd(mult, 4)
    Hp, Wp = fio.padded_size(h, w, mult)
    th, tw = (Hp, Wp) if tile is None else (min(tile[0], Hp), min(tile[1], Wp))
    ny, nx = len(tile_origins(Hp, th, overlap)), len(tile_origins(Wp, tw, overlap))
    n_tiles, nv, s = ny * nx, (4 if flip_test else 1), int(net.scale)
    plan = engine.StreamPlan(net._cfg(), th, tw, n_tiles * nv * stream_slots(int(net.nframes), in_flight, scenes))
    tile_out = 3 * s * th * s * tw * 4                       # one fuse tape's output
    return {'plan': plan, 'tile': (th, tw), 'grid': (ny, nx),
            'cache': plan.cache_bytes,
            'workspaces': in_flight * plan.workspace_bytes,
            'tile_buffers': in_flight * n_tiles * tile_out if n_tiles > 1 else 0,
            'staging': in_flight * 3 * s * Hp * s * Wp * 4,
            'flip': in_flight * (2 * 3 * th * tw * 4 + 4 * tile_out) if flip_test else 0}


_FOOTPRINT_TERMS = ('cache', 'workspaces', 'tile_buffers', 'staging', 'flip')


def tile_footprint(net, h, w, tile, overlap=16, in_flight=2, scenes=1, flip_test=False, multiple=4):
    """The bytes of every allocation that super_resolve_frames(net, h x w frames, tile=tile, tile_overlap=overlap, ...) makes for
    an EDVR network itself, from the stream plan's queries and without a GPU (the network may be on the CPU): the frame cache
    (n_tiles * nv * stream_slots slots of the tile's plan), one workspace per window in flight, and per window in flight the
    [n_tiles,3,s th,s tw] buffer of the fuse tapes' outputs (more than one tile), the stitched / fuse tape's [1,3,s Hp,s Wp]
    frame (the staging buffer, or the yielded tensor itself), and under flip_test the two [3,th,tw] mirror buffers and the
    four fuse outputs.  Not counted: the frames the caller holds, a frame's bytes on their way in, the yielded frames of
    `out` / `out_size` (a resampled frame and the encoder's bytes: a few times oh x ow), `scores`' workspace, and what the
    caching allocator rounds up.  tile=None: the whole frame as one tile.  `scenes`: 1, or any larger number for a video with
    cuts (stream_slots)."""
    parts = _tile_parts(net, h, w, tile, overlap, in_flight, scenes, flip_test, multiple)
    return sum(parts[k] for k in _FOOTPRINT_TERMS)


def choose_tile(net, h, w, budget, overlap=16, in_flight=2, scenes=1, flip_test=False, multiple=4):
    """(th, tw): the tile of the grid with the fewest tiles whose tile_footprint is at most `budget` bytes and whose plan passes
    the size check (StreamPlan.max_image_bytes < 2^32); among grids of one tile count the tile closest to square.  For a grid of
    ky x kx tiles the tile is the smallest that gives it: per axis the padded length itself (k = 1), or the smallest multiple of
    `multiple` (raised to a multiple of 4) >= (n + (k - 1) overlap) / k, at least 16 and 2 * overlap.  At most 16 tiles per axis
    are tried.  ValueError when no grid fits.  Host code."""
    from . import frames as fio
    _, overlap = _check_tile(None, overlap, who="choose_tile")
    mult = int(multiple) * (4 // math.gcd(int(multiple), 4))
    Hp, Wp = fio.padded_size(h, w, mult)

    def axis(n):
        found = {}
        for k in range(1, 17):
            t = n if k == 1 else max(-(-(n + (k - 1) * overlap) // (k * mult)) * mult, -(-16 // mult) * mult,
                                     -(-2 * overlap // mult) * mult)
            if t <= n and (k == 1 or t < n) and len(tile_origins(n, t, overlap)) == k:
                found.setdefault(k, t)
        return found
    ys, xs = axis(Hp), axis(Wp)
    grids = sorted(((ky * kx, abs(ys[ky] - xs[kx]), ys[ky], xs[kx]) for ky in ys for kx in xs))
    for _, _, th, tw in grids:
        parts = _tile_parts(net, h, w, (th, tw) if (th, tw) != (Hp, Wp) else None, overlap, in_flight, scenes, flip_test, mult)
        if parts['plan'].max_image_bytes < MAX_IMAGE_BYTES and sum(parts[k] for k in _FOOTPRINT_TERMS) <= budget:
            return th, tw
    raise ValueError("choose_tile: no grid of at most 16 x 16 tiles of a %d x %d frame fits %d bytes (overlap %d, in_flight %d)"
                     % (h, w, int(budget), overlap, max(1, int(in_flight))))


def _frame_format(who, frames, layout, out, multiple, pad_mode, matrix, yuv_range, out_size, sr_scale, default_multiple,
                  multiple_of):
    """The front end's checks of a video that is taken as a decoder delivers it, shared by super_resolve_frames and
    adapt_frames: (lay, h, w, out_fmt, Hp, Wp, out_size, mult) -- the frames' layout and size, the format of the yielded frames,
    the padded size, `out_size` (None where it is the SR frame's own size) and the multiple the frames are padded to
    (`multiple`, None: default_multiple; raised to a multiple of `multiple_of`).  ValueError for anything else; no GPU call."""
    from . import frames as fio
    lay, h, w = _video_format(frames, layout, who)
    if out not in (None, 'float', 'hwc_rgb', 'hwc_bgr') and not fio.is_yuv(out):
        raise ValueError("%s: out=%r (None, 'float', 'hwc_rgb', 'hwc_bgr' or one of %s)" % (
            who, out, ', '.join(fio.ALL_YUV_LAYOUTS)))
    fio.check_yuv_names(matrix, yuv_range)
    out_fmt = out if out is not None else ('float' if lay == 'chw' else lay)
    if out_size == (sr_scale * h, sr_scale * w):
        out_size = None                           # the SR frame's own size: today's calls
    if out_size is not None:
        fio.check_resize(sr_scale * h, sr_scale * w, out_size, "%s: out_size" % who)
    if fio.is_yuv(out_fmt):
        oh, ow = out_size if out_size is not None else (sr_scale * h, sr_scale * w)
        if fio.packed_needs(out_fmt, oh, ow):
            raise ValueError("%s: a packed %s output of %d x %d needs %s%s" % (
                who, out_fmt, oh, ow, fio.packed_needs(out_fmt, oh, ow), " (out_size)" if out_size is not None else ""))
    if h < 4 or w < 4:
        raise ValueError("%s: frames of %d x %d (at least 4 x 4)" % (who, h, w))
    mult = int(multiple) if multiple is not None else int(default_multiple)
    if mult < 1:
        raise ValueError("%s: multiple=%r must be positive" % (who, multiple))
    if mult % multiple_of:
        mult *= multiple_of // math.gcd(mult, multiple_of)   # the EDVR plans and the tile grid take multiples of 4 only
    Hp, Wp = fio.padded_size(h, w, mult)
    fio.check_pad(h, w, Hp, -(-Wp // 4) * 4, pad_mode)
    return lay, h, w, out_fmt, Hp, Wp, out_size, mult


def _check_scores(who, scores, T, name="scores"):
    if not (torch.is_tensor(scores) and scores.dtype == torch.float64 and tuple(scores.shape) == (T, 2)
            and scores.is_cuda and scores.is_contiguous()):
        raise ValueError("%s: gt needs %s, a contiguous float64 [%d, 2] tensor on the GPU" % (who, name, T))


def _frame_scoring(who, T, gt, gt_layout, scores, score, crop_border, out_fmt, out_size, sr_scale, h, w, matrix, yuv_range):
    """The checks of the `gt` arguments of the two frame generators, and score_into(i, sr, into=scores): row i of `into` from
    the frame about to be yielded, on the current stream.  None without `gt`.  ValueError for anything else; no GPU call."""
    from . import frames as fio
    if gt is None:
        if scores is not None:
            raise ValueError("%s: scores without gt" % who)
        return None
    if len(gt) != T:
        raise ValueError("%s: gt has %d frames, the video %d" % (who, len(gt), T))
    glay, gh, gw = _video_format(gt, gt_layout, who)
    olay = 'chw' if out_fmt == 'float' else out_fmt
    oh, ow = out_size if out_size is not None else (sr_scale * h, sr_scale * w)
    fio.check_score((olay, oh, ow), (glay, gh, gw), score, crop_border, (0, 1), "%s: gt" % who)
    if fio.is_yuv(olay) and not fio.is_yuv(glay) and (matrix, yuv_range) != ('bt601', 'limited'):
        raise ValueError("%s: the Y plane of a %s output is the Y8 of an RGB gt for matrix='bt601', "
                         "yuv_range='limited' alone, not for %r, %r" % (who, olay, matrix, yuv_range))
    _check_scores(who, scores, T)

    def score_into(i, sr, into=scores):
        fio.score(sr[0] if olay == 'chw' else sr, gt[i], olay, glay, channel=score, crop_border=crop_border, out=into[i])
    return score_into


def _finish_frame(who, sr, geometry, out_fmt, out_size, sr_scale, matrix, yuv_range, i=None, score_into=None, into=None):
    """The back end of the two frame generators for a network output sr [1,3,s Hp,s Wp] of a frame that was padded from
    h x w to Hp x Wp (geometry): frame i as it is yielded -- the s h x s w crop, resampled to `out_size` and converted to
    `out_fmt` -- and its score, on the current stream."""
    from . import frames as fio
    h, w, Hp, Wp = geometry
    s = sr.shape[-2] // Hp
    if out_size is not None:
        if s != sr_scale:
            raise RuntimeError("%s: the network scales by %d, opt['scale'] says %d" % (who, s, sr_scale))
        if out_fmt == 'float':
            sr = fio.resize(sr, s * h, s * w, out_size)[None]
        else:
            sr = fio.emit(sr, s * h, s * w, out_fmt, matrix=matrix, yuv_range=yuv_range, size=out_size)
    elif out_fmt == 'float':
        sr = sr if (Hp, Wp) == (h, w) else fio.emit(sr, s * h, s * w, 'chw')[None]
    else:
        sr = fio.emit(sr, s * h, s * w, out_fmt, matrix=matrix, yuv_range=yuv_range)
    if score_into is not None:
        if into is None:
            score_into(i, sr)                      # (behind the conversion, on the caller's stream like it)
        else:
            score_into(i, sr, into)
    return sr


def super_resolve_frames(opt, net, frames, padding='new_info', in_flight=2, *, layout=None, out=None, pad_mode='reflect',
                         multiple=None, matrix='bt601', yuv_range='limited', cuts=None, cut_threshold=10.0, out_size=None,
                         flip_test=False, gt=None, gt_layout=None, score='rgb', crop_border=0, scores=None,
                         tile=None, tile_overlap=16, tile_budget=None):
    """Super-resolves a VIDEO: `frames` is a [T,3,H,W] tensor or a list of [3,H,W] frames (CPU or GPU); yields the SR frame
    [1,3,sH,sW] of every frame, in order -- what `net(frames[index_generation(i, T, nframes, padding)][None])` gives, the
    sliding-window test of the reference's video datasets (video_test_dataset_int.py:219, `padding: new_info` in the
    shipped YAMLs), without the caller cutting clips.

    EDVR: consecutive windows share all but one frame, and everything up to L3_fea depends on one frame alone, so every
    frame's L1 / L2 / L3 features are extracted ONCE into a cache of nframes + in_flight - 1 slots (engine.StreamPlan,
    stream_schedule) and each window runs one gather launch + the tape from PCD alignment on.  `in_flight` windows are on
    the GPU at a time, one HIP stream each (the caller's and _clip_streams' further ones); a window's extractions run on
    its own stream.  Two kinds of events order the cache: frame extracted -> the windows that gather it, and window done
    -> the extraction that overwrites one of its slots (the cache is read by the gather alone, at the start of a window;
    by stream_schedule's capacity the windows concerned finished long before).  Extraction at batch 1 may pick other kernel
    kinds than the batch of a whole clip, so results match the per-clip forward at the parity bar, not bit for bit; they
    do not depend on in_flight.
    Any other network (TOFlow, DUF): the windows are built here and run by super_resolve_video -- same interface, no cache.
    A yielded frame stays valid until the generator is advanced `in_flight` times; frames and results are ordered against
    the caller's current stream.

    What a decoder delivers is accepted as it is (frames.py, csrc/frame_io.hip): `frames` may also be uint8 [T,H,W,3|4] or
    a list of [H,W,3|4] in RGB or BGR order (`layout`: 'chw' | 'hwc_rgb' | 'hwc_bgr'; None = 'chw' for float frames,
    'hwc_rgb' for uint8), pitched and offset views passed by stride, CPU frames copied to the device as bytes; and any
    H, W >= 4: a frame is padded at the bottom and right from itself (`pad_mode` 'reflect' | 'replicate', the modes of
    torch.nn.functional.pad) to a multiple of `multiple` (None: 4 for EDVR, 1 for other networks; 16 for TOFlow), and the
    SR frame is cropped back to s*H x s*W.  `out`: None keeps [1,3,sH,sW] fp32 for float frames and gives uint8
    [sH,sW,3] on the device in the input's channel order for uint8 frames (util.tensor2img's image); 'float', 'hwc_rgb',
    'hwc_bgr' force one.  Float planar frames that need no padding, with `out` unset, take exactly the calls described
    above (the crop / conversion otherwise runs as one more launch on the window's stream, out of a per-stream staging
    buffer).
    What a VIDEO decoder delivers is YCbCr 4:2:0 (frames.py, csrc/frame_yuv.hip): with `layout` 'nv12' or 'i420' (never
    inferred) `frames` is a uint8 [T, H*3/2, W] tensor or a list of packed frames or of plane tuples, converted with `matrix`
    ('bt601' | 'bt709') and `yuv_range` ('limited' | 'full') in the launch that fills the frame cache; `out` None then
    yields packed uint8 [sH*3/2, sW] frames of the input's layout on the device, written from the fp32 SR frame in one launch,
    and 'nv12' / 'i420' force such an output for RGB and float inputs too (sH and sW must be even).
    High-bit-depth video (HEVC Main10, AV1, VP9 profile 2): `layout` 'p010' / 'p012' (semi-planar, the level in the top bits of a
    16-bit word) or 'i420p10' / 'i420p12' (yuv420p10le / yuv420p12le), as uint16 or int16 tensors shaped like their 8-bit
    counterparts (csrc/frame_yuv.hip too); `out` None then yields packed torch.uint16 frames of the input's layout, quantised
    from the fp32 SR frame to 1024 / 4096 levels, and the four names force such an output for any input -- an 8-bit source can
    leave with 10 bits.
    Footage that is not 4:2:0 (frames.py): `layout` and `out` also take the 4:2:2 names 'i422' / 'nv16' / 'i422p10' /
    'i422p12' / 'p210' / 'p212' (packed [T, 2H, W] or planes; a packed output needs an even sW or `out_size` width alone) and the
    4:4:4 names 'i444' / 'i444p10' / 'i444p12' (packed [T, 3H, W]; any size), the 16-bit ones as the output of any input;
    everything said of the 4:2:0 layouts holds for them.
    A video of several scenes: `cuts` (None: one scene, the calls of before) lists the first frame of every new scene, or is
    'auto' for frames.detect_cuts(frames, layout, threshold=cut_threshold); no window then crosses a cut (video_windows), so
    every scene comes out as if it had been passed alone, and the frame cache has stream_slots' capacity.
    A target output size: with `out_size` = (oh, ow) every yielded frame is oh x ow instead of sH x sW, for every network and
    every `out` ('float': [1,3,oh,ow]; a packed 4:2:0 output needs oh and ow even, sH and sW no longer).  The SR frame's
    sH x sW crop -- never the padding around it -- is resampled on the device (frames.resize: separable antialiased bicubic,
    torch's interpolate(mode='bicubic', antialias=True); per axis sH / oh <= 4 and oh / sH <= 2) by one more launch on the
    window's stream, in front of the conversion.  None, or (sH, sW) itself, takes exactly the calls described above.
    More GPU time for a better frame: `flip_test` = True is the reference's x4 self-ensemble (`flip_test` of
    test_Vid4_REDS4_with_GT.py, util.flipx4_forward; EDVR's published "with self-ensemble" numbers) -- the network runs on
    every window as it is, mirrored in W, in H and in both, and the un-flipped outputs are averaged, (((y0 + flipW(y1)) +
    flipH(y2)) + flipHW(y3)) / 4 in this order (frames.flip / frames.flip_mean, csrc/frame_flip.hip).  EDVR: the
    frame cache holds 4 x stream_slots slots, variant v (0 none, 1 W, 2 H, 3 both) of frame f in slot v * slots + f % slots;
    a frame is still extracted once per variant -- variant 0 by the call above, the others from frames.flip of the PADDED
    fp32 frame (the network sees flip(pad(x)): the padding stays at the bottom and right of the source) -- and a window runs
    four fuse tapes and one flip_mean that writes the tensor the single fuse tape writes otherwise, so crop, `out_size`,
    every `out` and `cuts` work as described.  Other networks: super_resolve_video(flip_test=True), which needs a (padded)
    width that is a multiple of 4.  False takes exactly the calls described above: no further plan, buffer or launch.  Not
    provided: the x8 ensemble with transposes (a transposed frame needs a second plan of W x H), and flip-test inside
    Video_base_model.test() or the adaptation loops.
    How good the frames are: `gt` is a video of T ground-truth frames of the OUTPUT's size (sH x sW, or `out_size`), a tensor or
    a list like `frames`, in any layout frames.score takes (`gt_layout`; None: by dtype), on the CPU or the GPU, and `scores` a
    float64 [T, 2] tensor on the GPU (required with `gt`).  Row i becomes [mse, ssim] of frames.score(yielded frame i, gt[i],
    channel=`score`, crop_border=`crop_border`) (csrc/frame_score.hip), launched on the window's stream behind the
    launch that produced the frame and ordered against the caller's stream exactly like the frame: what is scored is the frame
    the caller gets -- the bytes of a uint8 output, emit()'s 8-bit image of a 'float' one, the Y plane of a 4:2:0 output
    (`score` = 'y' alone; the 10- / 12-bit levels of a 16-bit one, against a GT of that depth).  A 4:2:0 output scored in 'y'
    against an RGB GT needs matrix='bt601', yuv_range='limited': the only pair for which the Y plane is the Y8 of the GT.
    score_summary turns `scores` into the reference's per-scene PSNR / SSIM means.  The yielded frames are what they are
    without `gt`; None takes exactly the calls described above.
    Frames too large for one plan: the kernels address one image of a tensor with 32-bit offsets, so an EDVR plan whose largest
    per-image tensor (engine.StreamPlan.max_image_bytes: 4096 h w bytes for nf = 64 at scale 4) reaches 2^32 -- 1080 x 1920 does
    -- is refused with a ValueError that names `tile`, and the workspace of a plan grows with its pixels.  `tile` = (th, tw), an
    int for both, or 'auto' (None: the whole frame, exactly the calls described above) cuts the padded frame into overlapping
    tiles of ONE size, th x tw LR pixels (multiples of 4 and of `multiple`, at least 16 and 2 * tile_overlap), tile_origins
    per axis with `tile_overlap` LR pixels (a multiple of 4; 16 is a policy default, not tuned on real footage) shared by
    neighbours; a tile >= the frame on both axes is the whole frame again.  The frame that goes into the crop / `out_size` /
    `out` / `gt` chain above is then frames.stitch (csrc/frame_stitch.hip) of, for every tile, what
    super_resolve_frames(..., out='float') gives for the video of that tile's view [y : min(y + th, h), x : min(x + tw, w)] of
    every frame (frames.tile_view; only a tile at the bottom or right edge is padded, from itself) -- a linear cross-fade over
    the overlaps.  It is NOT the whole-frame output: EDVR's receptive field is larger than any overlap.  EDVR: one plan of
    th x tw with n_tiles * nv * slots cache slots, tile t's variant v of frame f in slot (t * nv + v) * slots + f % slots; a CPU
    frame crosses the bus once and every tile view is extracted from it; a window runs the tiles' fuse tapes (and flip_mean per
    tile under flip_test) into a per-stream [n_tiles,3,s th,s tw] buffer and one stitch launch writes the tensor the single fuse
    tape writes otherwise, all on the window's stream.  Other networks: the tiles run as clips through super_resolve_video and
    are stitched on the caller's stream; with `tile` set `multiple` is raised to a multiple of 4.  'auto' is
    choose_tile(net, h, w, tile_budget, ...) (EDVR), `tile_budget` bytes or, None, 0.8 x the free device memory -- a policy value.
    Arguments are checked before the first GPU call (ValueError)."""
    from . import frames as fio
    from .models.archs.EDVR_arch import EDVR
    T = len(frames)
    if T < 1:
        raise ValueError("super_resolve_frames: no frames")
    _check_flip_test(flip_test, "super_resolve_frames")
    in_flight = max(1, int(in_flight))
    is_edvr = isinstance(net, EDVR)
    if pad_mode not in ('reflect', 'replicate'):
        raise ValueError("super_resolve_frames: pad_mode=%r ('reflect' or 'replicate')" % (pad_mode,))
    # float frames with none of the frame arguments given, at a size the network takes as it is: the calls of before
    plain = layout is None and out is None and multiple is None and \
        torch.is_tensor(frames[0]) and frames[0].dtype not in (torch.uint8, torch.uint16, torch.int16)
    if is_edvr:
        plain = plain and torch.is_tensor(frames[0]) and frames[0].dim() == 3 and frames[0].is_floating_point() and \
            frames[0].shape[-2] % 4 == 0 and frames[0].shape[-1] % 4 == 0
    sr_scale = int(net.scale) if is_edvr else int(opt.get('scale') or 1)
    if out_size is not None:
        out_size = fio.check_size(out_size, "super_resolve_frames: out_size")
    tile, tile_overlap = _check_tile(tile, tile_overlap, tile_budget)
    if tile == 'auto' and not is_edvr:
        raise ValueError("super_resolve_frames: tile='auto' sizes an EDVR stream plan; pass (th, tw) for %s" % type(net).__name__)
    plain = plain and out_size is None and tile is None
    if plain:
        h, w, lay, out_fmt, Hp, Wp = int(frames[0].shape[-2]), int(frames[0].shape[-1]), 'chw', 'float', None, None
    else:
        lay, h, w, out_fmt, Hp, Wp, out_size, mult = _frame_format(
            "super_resolve_frames", frames, layout, out, multiple, pad_mode, matrix, yuv_range, out_size, sr_scale,
            4 if is_edvr else 1, 4 if is_edvr or tile is not None else 1)
    score_into = _frame_scoring("super_resolve_frames", T, gt, gt_layout, scores, score, crop_border, out_fmt, out_size,
                                sr_scale, h, w, matrix, yuv_range)
    n = int(net.nframes) if is_edvr or not (opt.get('network_G') or {}).get('nframes') else int(opt['network_G']['nframes'])
    if isinstance(cuts, str):
        if cuts != 'auto':
            raise ValueError("super_resolve_frames: cuts=%r (None, 'auto' or a sequence of frame numbers)" % (cuts,))
        video_windows(T, n, padding, [])                           # (the mode, before the first GPU call)
        cuts = fio.detect_cuts(frames, lay, threshold=cut_threshold)
    elif cuts is not None:
        cuts = [a for a, _ in scene_bounds(T, cuts)][1:]
    grid = None                                       # (th, tw, the tiles' origins per axis): more than one tile
    if tile is not None:
        if tile == 'auto':
            video_windows(T, n, padding, cuts)        # (the last check, in front of a query of the device's free memory)
            budget = tile_budget if tile_budget is not None else 0.8 * torch.cuda.mem_get_info(next(net.parameters()).device)[0]
            tile = choose_tile(net, h, w, budget, tile_overlap, in_flight, 1 if cuts is None else len(cuts) + 1, flip_test, mult)
        th, tw = min(tile[0], Hp), min(tile[1], Wp)
        if (th < Hp and th % mult) or (tw < Wp and tw % mult):
            raise ValueError("super_resolve_frames: tile=%r must be a multiple of multiple=%d" % (tuple(tile), mult))
        ys, xs = tile_origins(Hp, th, tile_overlap), tile_origins(Wp, tw, tile_overlap)
        if len(ys) * len(xs) > 1:
            grid = (th, tw, ys, xs)
            fio.check_pad(h - ys[-1], w - xs[-1], th, tw, pad_mode)     # the tile at the bottom right is padded from itself
    if not plain and grid is None and lay == 'chw' and out_fmt == 'float' and (Hp, Wp) == (h, w) and out_size is None:
        Hp = Wp = None                                # nothing to convert, pad or crop: today's calls
    if not is_edvr:
        windows, _ = video_windows(T, n, padding, cuts)            # (validates T, the mode and the cuts)
        if flip_test and (w if Hp is None else Wp) % 4:
            raise ValueError("super_resolve_frames: flip_test needs a width that is a multiple of 4, got %d (pass multiple=4)"
                             % (w if Hp is None else Wp))
        if Hp is None:
            def clips():
                for win in windows:
                    yield torch.stack([frames[j] for j in win])[None]
            if score_into is None:
                yield from super_resolve_video(opt, net, clips(), in_flight, flip_test)
                return
            for i, sr in enumerate(super_resolve_video(opt, net, clips(), in_flight, flip_test)):
                score_into(i, sr)                      # (on the caller's stream, which the frame is ordered against)
                yield sr
            return
        def finished(i, sr):
            return _finish_frame("super_resolve_frames", sr, (h, w, Hp, Wp), out_fmt, out_size, sr_scale, matrix, yuv_range,
                                 i, score_into)
        if grid is not None:
            # every window as n_tiles clips, tile by tile, through super_resolve_video; their outputs are copied into one
            # buffer and stitched on the caller's stream, which the clips' outputs are ordered against
            th, tw, ys, xs = grid
            origins = [(y, x) for y in ys for x in xs]
            first = frames[0] if torch.is_tensor(frames[0]) else frames[0][0]
            dev = first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device())
            on_device, kept = {}, {}                   # frame -> the frame on the device; (frame, tile) -> the ingested tile

            def ingested_tile(j, t):
                x = kept.get((j, t))
                if x is None:
                    if j not in on_device:
                        on_device[j] = fio.to_device(frames[j], dev)   # (a CPU frame crosses the bus once)
                        while len(on_device) > 2 * n:
                            on_device.pop(next(iter(on_device)))
                    x = kept[(j, t)] = fio.ingest(fio.tile_view(on_device[j], lay, origins[t][0], origins[t][1], th, tw), lay,
                                                  mult, pad_mode, matrix=matrix, yuv_range=yuv_range)
                    while len(kept) > 2 * n * len(origins):
                        kept.pop(next(iter(kept)))
                return x

            def tile_clips():
                for win in windows:
                    for t in range(len(origins)):
                        yield torch.stack([ingested_tile(j, t) for j in win])[None]
            tiles_sr = super_resolve_video(opt, net, tile_clips(), in_flight, flip_test)
            tables = None
            for i in range(T):
                buf = None
                for t in range(len(origins)):
                    sr = next(tiles_sr)
                    if buf is None:
                        s = sr.shape[-2] // th
                        if tuple(sr.shape) != (1, 3, s * th, s * tw) or s < 1:
                            raise RuntimeError("super_resolve_frames: a %d x %d tile came back as %s" % (th, tw, tuple(sr.shape)))
                        buf = torch.empty((len(origins), 3, s * th, s * tw), dtype=torch.float32, device=sr.device)
                        if tables is None:
                            tables = (fio.stitch_table(Hp, th, tile_overlap, s), fio.stitch_table(Wp, tw, tile_overlap, s))
                    buf[t].copy_(sr[0])
                yield finished(i, fio.stitch(buf, len(ys), len(xs), tables[0], tables[1])[None])
            return
        kept = {}                                      # frame -> its ingested tensor; the last 2n are kept

        def ingested(j):
            x = kept.get(j)
            if x is None:
                x = kept[j] = fio.ingest(frames[j], lay, mult, pad_mode, matrix=matrix, yuv_range=yuv_range)
                while len(kept) > 2 * n:
                    kept.pop(next(iter(kept)))
            return x

        def padded_clips():
            for win in windows:
                yield torch.stack([ingested(j) for j in win])[None]
        for i, sr in enumerate(super_resolve_video(opt, net, padded_clips(), in_flight, flip_test)):
            yield finished(i, sr)
        return
    leaves = net.ordered_parameters()
    dev = leaves[0].device
    sched = list(stream_schedule(T, net.nframes, padding, in_flight, cuts))
    direct = Hp is None                               # fp32 planar frames of the plan's size in, the fuse tape's tensor out
    ph, pw = (h, w) if direct else (Hp, Wp)
    slots = stream_slots(net.nframes, in_flight, 1 if cuts is None else len(cuts) + 1)
    nv = 4 if flip_test else 1                        # variants of a frame in the cache: slot v * slots + f % slots
    # the tiles: one plan of the tile's size, tile t's variant v of frame f in slot (t * nv + v) * slots + f % slots
    pth, ptw, origins = (ph, pw, [(0, 0)]) if grid is None else (grid[0], grid[1], [(y, x) for y in grid[2] for x in grid[3]])
    n_t = len(origins)
    plan = engine.get_stream_plan(net._cfg(), pth, ptw, n_t * nv * slots, dev)
    if plan.max_image_bytes >= MAX_IMAGE_BYTES:       # (a host query: before the device check and the first GPU call)
        raise ValueError("super_resolve_frames: a %d x %d %s needs a tensor of %d bytes per image, and the kernels address an image "
                         "with 32-bit offsets (< 2^32 bytes): pass tile= (a smaller tile, or 'auto') to run it in tiles"
                         % (pth, ptw, "frame" if grid is None else "tile", plan.max_image_bytes))
    if dev.type != 'cuda':
        raise RuntimeError("dynavsr_amd EDVR runs on the MI355X only (the network is on %s); there is no CPU fallback" % dev)
    if Hp is None and tuple(frames[0].shape[-3:-2]) != (3,):
        raise RuntimeError("super_resolve_frames expects frames [3,H,W], got %s" % (tuple(frames[0].shape),))

    def sid(t, v, slot):
        return (t * nv + v) * slots + slot
    main = torch.cuda.current_stream(dev)
    streams = _clip_streams(dev, in_flight)
    with torch.cuda.device(dev):
        cache = plan.new_cache(dev)
    for s in streams[1:]:
        cache.record_stream(s)
    extracted, readers, pending = {}, {}, []   # slot -> event of its extraction; slot -> events of the windows reading it
    staging = {}                               # stream index -> the fuse tape's output when a crop / conversion follows it
    resized = {}                               # stream index -> the resampled frame when a conversion follows it
    flipped = {}                               # flip_test: stream index -> [the padded frame, one mirror image of it]
    fused = {}                                 # flip_test: stream index -> the four fuse tapes' outputs
    tiled = {}                                 # tiles: stream index -> the tiles' fuse outputs [n_t,3,s pth,s ptw]
    if grid is not None:
        with torch.cuda.device(dev):               # the blend tables of the two axes, on the device once per video
            axes = [fio._stitch_axis(fio.stitch_table(nn, tt, tile_overlap, int(net.scale)), dev)
                    for nn, tt in ((ph, pth), (pw, ptw))]

    def fuse_tile(k, t, wslots, dst):
        """Tile t of the window in `wslots` -> dst [1,3,s pth,s ptw] on the current stream (of index k): the fuse tape, or, with
        flip_test, the four variants' fuse tapes and the launch that un-flips and averages them."""
        if not flip_test:
            plan.fuse(leaves, [sid(t, 0, slot) for slot in wslots], cache, dst)
            return
        if k not in fused:
            fused[k] = [torch.empty_like(dst) for _ in range(nv)]
        for v in range(nv):
            plan.fuse(leaves, [sid(t, v, slot) for slot in wslots], cache, fused[k][v])
        fio.flip_mean(*fused[k], out=dst)

    def fuse(k, wslots, dst):
        """The window in `wslots` -> dst [1,3,s ph,s pw] on the current stream (of index k): fuse_tile, or every tile's into
        the stream's tile buffer and the launch that stitches them."""
        if grid is None:
            fuse_tile(k, 0, wslots, dst)
            return
        if k not in tiled:
            tiled[k] = torch.empty((n_t, 3, net.scale * pth, net.scale * ptw), dtype=torch.float32, device=dev)
        for t in range(n_t):
            fuse_tile(k, t, wslots, tiled[k][t:t + 1])
        fio._stitch_run(tiled[k], len(grid[2]), len(grid[3]), axes[0], axes[1], dst[0])
    was_training = net.training
    net.eval()
    try:
        for step, (centre, _, new, wslots) in enumerate(sched):
            if len(pending) == len(streams):
                sr, ev = pending.pop(0)
                main.wait_event(ev)
                sr.record_stream(main)
                yield sr
            s = streams[step % len(streams)]
            if s != main:
                s.wait_stream(main)                  # the frames (and the weights) were produced on the caller's stream
            with torch.cuda.stream(s), torch.no_grad():
                for f, slot in new:
                    x = frames[f]
                    if direct:
                        x = engine._prep(x if x.is_cuda else x.to(dev))
                    else:
                        x = fio.to_device(x, dev)                    # (8-bit frames travel as bytes)
                    for t in range(n_t):
                        for v in range(nv):
                            for ev in readers.pop(sid(t, v, slot), ()):
                                s.wait_event(ev)
                    read = []                         # the tensors the extraction launches read
                    for t, (ty, tx) in enumerate(origins):
                        xt = x if grid is None else fio.tile_view(x, lay, ty, tx, pth, ptw)
                        if flip_test:                 # the padded fp32 frame, then its mirror images one at a time
                            k = step % len(streams)
                            if k not in flipped:
                                flipped[k] = [torch.empty((3, pth, ptw), dtype=torch.float32, device=dev) for _ in range(2)]
                            if direct:
                                padded = xt if xt.data_ptr() % 16 == 0 else flipped[k][0].copy_(xt)
                            else:
                                padded = fio.ingest(xt, lay, mult, pad_mode, out=flipped[k][0], matrix=matrix, yuv_range=yuv_range)
                        if direct:
                            plan.extract(leaves, xt, sid(t, 0, slot), cache)
                        else:
                            xt = plan.extract_frame(leaves, xt, sid(t, 0, slot), cache, lay, pad_mode, matrix, yuv_range)
                        read += [xt] if torch.is_tensor(xt) else list(xt)
                        for v in range(1, nv):
                            plan.extract(leaves, fio.flip(padded, v, out=flipped[k][1]), sid(t, v, slot), cache)
                    ev = torch.cuda.Event()
                    ev.record(s)
                    for t in range(n_t):
                        for v in range(nv):
                            extracted[sid(t, v, slot)] = ev
                    if s != main:
                        for t in read:
                            t.record_stream(s)
                for ev in set(extracted[sid(t, v, slot)] for t in range(n_t) for v in range(nv) for slot in set(wslots)):
                    s.wait_event(ev)
                if direct or (out_fmt == 'float' and (ph, pw) == (h, w) and out_size is None):
                    sr = torch.empty((1, 3, net.scale * ph, net.scale * pw), dtype=torch.float32, device=dev)
                    fuse(step % len(streams), wslots, sr)
                else:
                    k = step % len(streams)
                    if k not in staging:
                        staging[k] = torch.empty((1, 3, net.scale * ph, net.scale * pw), dtype=torch.float32, device=dev)
                    fuse(k, wslots, staging[k])
                    if out_size is not None and out_fmt == 'float':
                        sr = fio.resize(staging[k], net.scale * h, net.scale * w, out_size)[None]
                    elif out_size is not None:
                        if k not in resized:
                            resized[k] = fio.resize_buffer(out_size, dev)
                        fio.resize(staging[k], net.scale * h, net.scale * w, out_size, out=resized[k])
                        sr = fio.emit(resized[k], out_size[0], out_size[1], out_fmt, matrix=matrix, yuv_range=yuv_range)
                    elif out_fmt == 'float':
                        sr = fio.emit(staging[k], net.scale * h, net.scale * w, 'chw')[None]
                    else:
                        sr = fio.emit(staging[k], net.scale * h, net.scale * w, out_fmt, matrix=matrix, yuv_range=yuv_range)
                if score_into is not None:
                    score_into(centre, sr)             # (behind the launch that wrote sr; the event below covers the row too)
                ev = torch.cuda.Event()
                ev.record(s)
            for slot in set(wslots):
                for t in range(n_t):
                    for v in range(nv):
                        readers.setdefault(sid(t, v, slot), []).append(ev)
            pending.append((sr, ev))
        while pending:
            sr, ev = pending.pop(0)
            main.wait_event(ev)
            sr.record_stream(main)
            yield sr
    finally:
        # a generator closed early leaves windows running on the side streams: whatever the caller does next on its stream
        # (an update of the weights they read, the release of the cache) must come behind them
        for sr, ev in pending:
            main.wait_event(ev)
            sr.record_stream(main)
        net.train(was_training)


def adapt_multiple(opt):
    """The multiple of its sides at which a clip can be adapted: the backbone runs on the clip and on its SLR version, 1 / scale
    the size.  EDVR takes multiples of 4, so 4 * scale; TOFlow multiples of 16 at the clip's size, where it also sees the SLR
    clip (backbone_input), so lcm(scale, 16); DUF any size, so scale.  Host code."""
    which = (opt['network_G'] or {}).get('which_model_G')
    s = int(opt['scale'])
    if which == 'EDVR':
        return 4 * s
    if which == 'TOF':
        return s * 16 // math.gcd(s, 16)
    if which == 'DUF':
        return s
    raise ValueError("adapt_multiple: network_G.which_model_G=%r (EDVR, TOF or DUF)" % (which,))


def adapt_frames(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, frames, padding='new_info', *, layout=None,
                 out=None, pad_mode='reflect', multiple=None, matrix='bt601', yuv_range='limited', cuts=None,
                 cut_threshold=10.0, out_size=None, gt=None, gt_layout=None, score='rgb', crop_border=0, scores=None,
                 baseline_scores=None, losses=None, baseline=True, overlap=True, frames_per_batch=1):
    """Test-time adaptation of a decoded VIDEO (test_dynavsr.py:197-283 without the caller cutting, cropping or converting
    clips): for every frame, in order, yields (baseline frame | None, adapted frame) -- the un-adapted network's output and the
    output of the copies adapted on that frame's window, both in the format super_resolve_frames would yield for the same
    `layout` / `out` / `out_size`.

    Front end: `frames`, `layout`, `matrix`, `yuv_range` as in super_resolve_frames -- uint8 RGB / BGR, every YCbCr layout at
    8 / 10 / 12 bits, float planar, CPU or GPU, of any size.  Every frame goes through frames.ingest once, on the device, padded
    at the bottom and right (`pad_mode`) to a multiple of `multiple` (None: M = adapt_multiple(opt); a caller's value must be
    a multiple of M); the last 2 * nframes ingested frames are kept.  The windows are video_windows(T, nframes, padding, cuts)
    (`cuts` = 'auto': frames.detect_cuts), the clips torch.stack of the ingested frames.
    Middle: adapt_video(clips, overlap, frames_per_batch, region=(h, w), baseline=baseline), unchanged otherwise.  The padded
    band holds copies of real pixels, so the objective counts the frame's own h x w alone (adapt_frame's `region`; left out
    when the frame needed no padding).  baseline=False skips the un-adapted forward -- a third of a frame's device time -- and
    yields None in its place.
    Back end: the SR frame's s h x s w crop through frames.resize (`out_size`) and frames.emit, on the caller's stream.  With
    `gt` (a video of T frames of the output's size) row i of `scores` becomes [mse, ssim] of frames.score(adapted frame i,
    gt[i]) and row i of `baseline_scores` (optional; needs baseline=True) that of the baseline frame, with the argument rules of
    super_resolve_frames (float64 [T, 2] GPU tensors; score_summary reads them).  `losses`: an optional float32
    [T, train.maml.adapt_iter] GPU tensor; row i receives frame i's per-step losses without a host synchronisation.

    A yielded pair stays valid until the generator is advanced 2 * max(1, frames_per_batch) times: where nothing is cropped,
    resampled or converted (float output of an unpadded frame) the pair is adapt_video's own, which holds its rule; every other
    pair is a tensor of its own.  Frames and results are ordered against the caller's current stream.
    Not provided: train.use_real (the reference reads ready-made SLR images from disk there); `tile` and `flip_test`; frames
    whose EDVR plan reaches the 4 GiB image limit (ValueError); adapting once per scene; chroma-only adaptation.
    Arguments are checked before the first GPU call (ValueError)."""
    from . import frames as fio
    who = "adapt_frames"
    if opt['train']['use_real']:
        raise ValueError("adapt_frames: train.use_real reads ready-made SLR clips ('SuperLQs'), which a decoded video does not "
                         "have; pass clips to adapt_video")
    T = len(frames)
    if T < 1:
        raise ValueError("adapt_frames: no frames")
    if pad_mode not in ('reflect', 'replicate'):
        raise ValueError("adapt_frames: pad_mode=%r ('reflect' or 'replicate')" % (pad_mode,))
    M = adapt_multiple(opt)
    if multiple is not None and (isinstance(multiple, bool) or int(multiple) < 1 or int(multiple) % M):
        raise ValueError("adapt_frames: multiple=%r must be a multiple of %d (adapt_multiple)" % (multiple, M))
    sr_scale = int(opt['scale'])
    if out_size is not None:
        out_size = fio.check_size(out_size, "adapt_frames: out_size")
    lay, h, w, out_fmt, Hp, Wp, out_size, mult = _frame_format(who, frames, layout, out, multiple, pad_mode, matrix, yuv_range,
                                                               out_size, sr_scale, M, 1)
    score_into = _frame_scoring(who, T, gt, gt_layout, scores, score, crop_border, out_fmt, out_size, sr_scale, h, w, matrix,
                                yuv_range)
    if baseline_scores is not None:
        if not baseline:
            raise ValueError("adapt_frames: baseline_scores needs the baseline frames (baseline=True)")
        if gt is None:
            raise ValueError("adapt_frames: baseline_scores without gt")
        _check_scores(who, baseline_scores, T, "baseline_scores")
    steps = int(opt['train']['maml']['adapt_iter'])
    if losses is not None:
        if not (torch.is_tensor(losses) and losses.dtype == torch.float32 and tuple(losses.shape) == (T, steps)):
            raise ValueError("adapt_frames: losses must be a float32 [%d, %d] tensor (frames x train.maml.adapt_iter)" % (T, steps))
        if not (losses.is_cuda and losses.is_contiguous()):
            raise ValueError("adapt_frames: losses must be contiguous and on the GPU")
    n = (opt['network_G'] or {}).get('nframes')
    if not n:
        raise ValueError("adapt_frames: network_G.nframes, the length of a window, is not set")
    n = int(n)
    region = check_adapt_region(opt, (3, Hp, Wp), (h, w))         # (None where the frame needs no padding)
    from .models.archs.EDVR_arch import EDVR
    if isinstance(getattr(model, 'netG', None), EDVR):
        # (a host query of a stream plan that is never run: the tapes of the loops hold the same per-image tensors)
        need = engine.StreamPlan(model.netG._cfg(), Hp, Wp, int(model.netG.nframes)).max_image_bytes
        if need >= MAX_IMAGE_BYTES:
            raise ValueError("adapt_frames: a %d x %d frame needs a tensor of %d bytes per image, and the kernels address an "
                             "image with 32-bit offsets (< 2^32 bytes); adaptation in tiles is not provided" % (Hp, Wp, need))
    if isinstance(cuts, str):
        if cuts != 'auto':
            raise ValueError("adapt_frames: cuts=%r (None, 'auto' or a sequence of frame numbers)" % (cuts,))
        video_windows(T, n, padding, [])                           # (the mode, before the first GPU call)
        cuts = fio.detect_cuts(frames, lay, threshold=cut_threshold)
    elif cuts is not None:
        cuts = [a for a, _ in scene_bounds(T, cuts)][1:]
    windows, _ = video_windows(T, n, padding, cuts)
    kept = {}                                          # frame -> its ingested tensor; the last 2n are kept

    def ingested(j):
        x = kept.get(j)
        if x is None:
            x = kept[j] = fio.ingest(frames[j], lay, mult, pad_mode, matrix=matrix, yuv_range=yuv_range)
            while len(kept) > 2 * n:
                kept.pop(next(iter(kept)))
        return x

    def clips():
        for win in windows:
            yield {'LQs': torch.stack([ingested(j) for j in win])[None]}

    def finished(i, sr, into):
        return _finish_frame(who, sr, (h, w, Hp, Wp), out_fmt, out_size, sr_scale, matrix, yuv_range, i,
                             score_into if into is not None else None, into)
    results = adapt_video(opt, model, est_model, modelcp, est_modelcp, est_model_fixed, clips(), overlap=overlap,
                          frames_per_batch=frames_per_batch, region=region, baseline=baseline)
    for i, (base, r) in enumerate(results):
        if losses is not None:
            losses[i].copy_(torch.stack([l_.reshape(()) for l_ in r['losses']]))
        yield (finished(i, base, baseline_scores) if base is not None else None,
               finished(i, r['sr'], scores if score_into is not None else None))


def score_summary(scores, nframes, cuts=None, peak=255):
    """The reference's per-folder report (test_Vid4_REDS4_with_GT.py) from the [T, 2] rows [mse, ssim] that
    super_resolve_frames(gt=...) wrote: one device-to-host copy, then host arithmetic.

    A scene (scene_bounds(T, cuts); cuts=None: the whole video) plays the part of a folder.  With border_frame = nframes // 2,
    frame i of a scene of N frames is a centre frame when border_frame <= i < N - border_frame and a border frame otherwise.
    Per scene: 'psnr' / 'ssim' are the means of the per-frame values over all frames, '_center' / '_border' those over the two
    groups; a border mean over no frames is 0, like the reference, and a centre mean over no frames (a scene shorter than
    2 * border_frame, where the reference would divide by zero) is NaN.  The per-frame PSNR is frames.psnr(mse, peak): inf for
    identical frames.  Returns {'scenes': [{'first', 'frames', 'center_frames', 'border_frames', 'psnr', 'psnr_center',
    'psnr_border', 'ssim', 'ssim_center', 'ssim_border'}, ...], 'mean': the plain mean over scenes of the six values}."""
    from . import frames as fio
    rows = torch.as_tensor(scores).detach().to('cpu', torch.float64)
    if rows.dim() != 2 or rows.shape[1] != 2 or rows.shape[0] < 1:
        raise ValueError("score_summary: scores must be [T, 2], got %s" % (tuple(rows.shape),))
    nframes = int(nframes)
    if nframes < 1:
        raise ValueError("score_summary: nframes=%d must be positive" % nframes)
    rows = rows.tolist()
    border = nframes // 2

    def mean(v, empty):
        return sum(v) / len(v) if v else empty
    keys = ('psnr', 'psnr_center', 'psnr_border', 'ssim', 'ssim_center', 'ssim_border')
    scenes = []
    for a, b in scene_bounds(len(rows), [] if cuts is None else cuts):
        p = [fio.psnr(m, peak) for m, _ in rows[a:b]]
        s = [v for _, v in rows[a:b]]
        centre = [border <= i < (b - a) - border for i in range(b - a)]
        pc, pb = [v for v, c in zip(p, centre) if c], [v for v, c in zip(p, centre) if not c]
        sc, sb = [v for v, c in zip(s, centre) if c], [v for v, c in zip(s, centre) if not c]
        scenes.append({'first': a, 'frames': b - a, 'center_frames': len(pc), 'border_frames': len(pb),
                       'psnr': mean(p, 0.0), 'psnr_center': mean(pc, float('nan')), 'psnr_border': mean(pb, 0.0),
                       'ssim': mean(s, 0.0), 'ssim_center': mean(sc, float('nan')), 'ssim_border': mean(sb, 0.0)})
    return {'scenes': scenes, 'mean': {k: sum(sc[k] for sc in scenes) / len(scenes) for k in keys}}


def evaluate_frames(opt, net, frames, gt, **kw):
    """Drains super_resolve_frames(opt, net, frames, gt=gt, **kw) and returns (score_summary(scores, nframes, cuts, peak),
    scores): the evaluation scripts of the reference for one video.  `scores` (a float64 [T, 2] GPU tensor) is allocated on the
    network's device unless passed; cuts='auto' is resolved here, so that the summary has the scenes the windows had; `peak`
    (None: 255, or 2^d - 1 for a 10- / 12-bit output) goes to score_summary."""
    from . import frames as fio
    from .models.archs.EDVR_arch import EDVR
    kw = dict(kw)
    peak = kw.pop('peak', None)
    T = len(frames)
    if isinstance(kw.get('cuts'), str) and kw['cuts'] == 'auto':
        kw['cuts'] = fio.detect_cuts(frames, kw.get('layout'), threshold=kw.get('cut_threshold', 10.0))
    if kw.get('scores') is None:
        p = next(iter(net.parameters()), None)
        dev = p.device if p is not None and p.is_cuda else torch.device('cuda', torch.cuda.current_device())
        kw['scores'] = torch.zeros((T, 2), dtype=torch.float64, device=dev)
    scores = kw['scores']
    for _ in super_resolve_frames(opt, net, frames, gt=gt, **kw):
        pass
    n = int(net.nframes) if isinstance(net, EDVR) or not (opt.get('network_G') or {}).get('nframes') else \
        int(opt['network_G']['nframes'])
    if peak is None:
        o = kw.get('out') if kw.get('out') is not None else kw.get('layout')
        peak = 2 ** fio.layout_depth(o) - 1 if fio.is_yuv(o) else 255
    return score_summary(scores, n, kw.get('cuts'), peak), scores
