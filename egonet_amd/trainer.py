"""Training loops with the reference's signatures (``libs/trainer/trainer.py``:
``train`` :127-263, ``train_cascade`` :25-71, ``get_loader`` :112-125) around the
native training steps.

What is the reference's and stays on the host: the ``DataLoader``, epochs, the
learning-rate schedule (``MultiStepLR``, optimizer.py:8-40), logging, optional
metric callbacks, snapshots.  What is replaced: the five lines of its hot loop
(trainer.py:183-209, ``zero_grad / forward / loss / backward / step``) -- one call
of ``HRNetTrainStep.step`` / ``LifterTrainStep.step`` (HIP launches only).

``evaluate`` (trainer.py:395-513) is the reference's validation loop: ``model.eval()`` and
``model(data)`` with autograd enabled -- which here runs the HIP inference program (the modules
ignore the autograd mode in eval mode) -- then the caller's loss / evaluator objects.

``loss_func`` and ``optim`` are accepted like in the reference; they are read, not
executed: the loss weights come from ``loss_func.comp_dict`` when it has one
(JointsCompositeLoss, function.py:61-93) else from
``cfgs['heatmapModel']['loss_weight_list']``; the learning rate of every epoch is
read from ``optim.param_groups`` after ``sche.step()``.  For the 'angleregression' head
(exp_type baselinealpha / baselinetheta) the criterion's class name -- ``MSELoss1D`` / ``SmoothL1Loss1D``,
function.py:204-228 -- or ``cfgs['heatmapModel']['loss_type']`` selects the native step's ``angle_type``.  The reference's
debug pictures (``save_debug``, trainer.py:223-234 and :450-466) are composed on the device and written by a background
thread (``visualization/debug.py``); its loss-curve plotting is not reproduced.
"""
import gc
import os
import time

import numpy as np
import torch

from . import optim as optim_spec
from . import parallel
from .model import FCmodel
from .model.heatmapModel.hrnet import PoseHighResolutionNet
from .train_hrnet import HRNetTrainStep
from .train_lifter import LifterTrainStep
from .visualization import debug as debug_pictures


def get_loader(dataset, cfgs, split, collate_fn=None):
    setting = cfgs[split + '_settings']
    if hasattr(dataset, 'device_loader'):
        # rows that live on the device (common.lifter_pairs.LifterPairs): the same order as the DataLoader below
        # for the same torch seed, one row fetch per batch instead of worker processes and a host collate
        return dataset.device_loader(setting['batch_size'], setting['shuffle'])
    kw = dict(batch_size=setting['batch_size'], num_workers=setting['num_threads'], shuffle=setting['shuffle'])
    if collate_fn is not None:
        kw['collate_fn'] = collate_fn
    return torch.utils.data.DataLoader(dataset, **kw)


def _flag(o, key):
    """A boolean key of a config section (YAML booleans, or the strings a hand-written file may hold)."""
    v = o.get(key, False)
    if isinstance(v, str):
        return v.strip().lower() in ('true', 'yes', 'on', '1')
    return bool(v)


def prepare_optim(model, cfgs):
    """optimizer.py:8-40 -- the torch objects carry the schedule; the native step does the update."""
    o = cfgs['optimizer']
    params = [p for p in model.parameters() if p.requires_grad]
    wd = float(o.get('weight_decay', 0.0) or 0.0)
    # beyond the reference, all absent by default: optim_type 'adamw', amsgrad, nesterov, dampening, and
    # no_decay_norm_bias -- two groups, the conv / linear weights keep weight_decay, BatchNorm gamma / beta and all
    # biases get 0.  (max_grad_norm is read by make_step: it is the step's, not the torch object's.)
    if _flag(o, 'no_decay_norm_bias'):
        inner = model.module if hasattr(model, 'module') else model
        params = [g for g in optim_spec.no_decay_groups(inner, wd) if g['params']]
    if o['optim_type'] in ('adam', 'adamw'):
        cls = torch.optim.Adam if o['optim_type'] == 'adam' else torch.optim.AdamW
        more = dict(amsgrad=True) if _flag(o, 'amsgrad') else {}
        optim = cls(params, lr=o['lr'], weight_decay=wd, **more)
    elif o['optim_type'] == 'sgd':
        more = {}
        if _flag(o, 'nesterov'):
            more['nesterov'] = True
        if o.get('dampening'):
            more['dampening'] = float(o['dampening'])
        optim = torch.optim.SGD(params, lr=o['lr'], momentum=float(o.get('momentum', 0.0) or 0.0), weight_decay=wd,
                                **more)
    else:
        raise NotImplementedError(o['optim_type'])              # as the reference (optimizer.py:27-28)
    sche = torch.optim.lr_scheduler.MultiStepLR(optim, milestones=o['milestones'], gamma=o['gamma'])
    return optim, sche


def add_optim_arguments(ap):
    """The optimizer switches of tools/train_IGRs.py and tools/train_lifting.py (argparse)."""
    ap.add_argument('--optim', default='adam', choices=['adam', 'adamw', 'sgd'])
    ap.add_argument('--weight-decay', type=float, default=0.0)
    ap.add_argument('--no-decay-norm-bias', action='store_true',
                    help='no weight decay on BatchNorm gamma / beta and on biases (two parameter groups)')
    ap.add_argument('--max-grad-norm', type=float, default=None, metavar='X',
                    help='clip the gradient to this 2-norm inside the update (off by default)')


def optim_keys_from_args(args):
    """-> the keys of cfgs['optimizer'] the switches above set."""
    keys = {'optim_type': getattr(args, 'optim', 'adam'), 'weight_decay': getattr(args, 'weight_decay', 0.0)}
    if getattr(args, 'no_decay_norm_bias', False):
        keys['no_decay_norm_bias'] = True
    if getattr(args, 'max_grad_norm', None) is not None:
        keys['max_grad_norm'] = args.max_grad_norm
    return keys


def add_checkpoint_arguments(ap):
    """``--checkpoint FILE`` / ``--resume FILE`` of tools/train_IGRs.py and tools/train_lifting.py (argparse)."""
    ap.add_argument('--checkpoint', default=None, metavar='FILE',
                    help='write a training checkpoint (model, optimizer state, schedule, generators) after every epoch')
    ap.add_argument('--resume', default=None, metavar='FILE',
                    help='continue the run a training checkpoint holds, at the epoch after its last')


def checkpoint_keys_from_args(args):
    """-> the keys of cfgs['training_settings'] the two switches set (none when neither is given)."""
    keys = {}
    if getattr(args, 'checkpoint', None):
        keys.update(checkpoint=args.checkpoint, checkpoint_every=1)
    if getattr(args, 'resume', None):
        keys['resume'] = args.resume
    return keys


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _barrier():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


_HOST_GROUP = None


def _make_host_group():
    """The host-side (gloo) group the waiting ranks use during rank 0's validation, created ONCE at the start of
    ``train`` -- where every rank arrives together (``dist.new_group`` is itself a collective: made lazily at the first
    mid-epoch evaluation, ranks != 0 would sit in it for the whole validation and could time out while rank 0 is still
    evaluating).  False = could not be made (the default group's barrier is used)."""
    global _HOST_GROUP
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    if _HOST_GROUP is None:
        import datetime
        try:
            _HOST_GROUP = dist.new_group(backend='gloo', timeout=datetime.timedelta(hours=12))
        except Exception:
            _HOST_GROUP = False


def _wait_for_rank0():
    """Ranks != 0 wait here while rank 0 validates: a barrier of the host-side (gloo) group (12 h timeout) where it
    could be made -- a GPU barrier kernel would sit on the device for the whole validation and is subject to the NCCL
    watchdog timeout of the training group -- else the default group's barrier."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    _make_host_group()          # (a no-op after train()'s call; callers outside train() make it at their first wait)
    if _HOST_GROUP:
        dist.barrier(group=_HOST_GROUP)
    else:
        dist.barrier()


def _optim_kwargs(optim, cfgs):
    """optimizer family / momentum / weight decay of the native update, from the torch optimizer object
    ``prepare_optim`` made (or, without one, from cfgs['optimizer'])."""
    if optim is not None:
        g = optim.param_groups[0]
        # the native update is ONE launch over one flat buffer with one set of hyper-parameters: parameter
        # groups that differ (per-group weight decay / momentum / betas) cannot be collapsed silently
        keys = ('momentum', 'weight_decay', 'betas', 'eps', 'dampening', 'nesterov', 'amsgrad')
        for other in optim.param_groups[1:]:
            diff = [k for k in keys if other.get(k) != g.get(k)]
            if diff:
                raise NotImplementedError('native update: param_groups with different %s (one flat buffer, one '
                                          'set of hyper-parameters)' % ', '.join(diff))
        if isinstance(optim, torch.optim.SGD):
            if g.get('dampening', 0) or g.get('nesterov', False):
                raise NotImplementedError('SGD with dampening / Nesterov momentum')
            return dict(optim_type='sgd', momentum=float(g.get('momentum', 0.0)), weight_decay=float(g['weight_decay']))
        if isinstance(optim, torch.optim.Adam) and not isinstance(optim, torch.optim.AdamW):
            if g.get('amsgrad', False):
                raise NotImplementedError('Adam with amsgrad')
            return dict(optim_type='adam', betas=tuple(g['betas']), eps=float(g['eps']),
                        weight_decay=float(g['weight_decay']))
        raise NotImplementedError('native update for %s' % type(optim).__name__)
    o = cfgs['optimizer']
    return dict(optim_type=o.get('optim_type', 'adam'), momentum=float(o.get('momentum', 0.0) or 0.0),
                weight_decay=float(o.get('weight_decay', 0.0) or 0.0))


_CRITERION_NAMES = {'MSELoss': 'mse', 'L1Loss': 'l1', 'SmoothL1Loss': 'sl1'}      # loss_dict, function.py:17-20
_OFF = (None, 'None', 0, 0.0)


def _loss_weights(loss_func, cfgs):
    """(w_hm, w_coor, cross-ratio keywords of HRNetTrainStep) from a JointsCompositeLoss-like
    object (comp_dict / cr_indices / target_cr / cr_loss_thres, function.py:61-93 and
    train_IGRs.py:33-46) or, without one, from cfgs['heatmapModel']."""
    hm = cfgs.get('heatmapModel', {})
    comp = getattr(loss_func, 'comp_dict', None)
    if comp is not None:
        spec = [_CRITERION_NAMES.get(type(comp[k][0]).__name__, type(comp[k][0]).__name__) if k in comp else 'None'
                for k in ('hm', 'coor', 'cr')]
        wl = [comp[k][1] if k in comp else 'None' for k in ('hm', 'coor', 'cr')]
    else:
        wl = list(hm.get('loss_weight_list', [1.0, 0.1, 'None']))
        spec = list(hm.get('loss_spec_list', ['mse', 'l1', 'None']))
    for k in spec[:2]:
        if k not in ('mse', 'l1', 'sl1', 'None'):
            raise NotImplementedError('loss criterion %r (loss_dict knows mse, l1, sl1)' % (k,))
    w_hm = float(wl[0]) if spec[0] != 'None' else 0.0
    w_coor = float(wl[1]) if spec[1] != 'None' else 0.0
    cr = {}
    if spec[0] not in ('mse', 'None'):
        cr['hm_type'] = spec[0]          # keywords of HRNetTrainStep beyond the shipped mse / l1 pair
    if spec[1] not in ('l1', 'None'):
        cr['coor_type'] = spec[1]
    if spec[2] != 'None' and wl[2] not in _OFF:
        if spec[2] not in ('mse', 'l1', 'sl1'):
            raise NotImplementedError('cross-ratio criterion %r' % spec[2])
        cr.update(w_cr=float(wl[2]), cr_type=spec[2],
                  cr_indices=getattr(loss_func, 'cr_indices', None),
                  target_cr=getattr(loss_func, 'target_cr', None) or 4.0 / 3.0,
                  cr_loss_thres=getattr(loss_func, 'cr_loss_thres', hm.get('cr_loss_threshold', 0.15)))
    return w_hm, w_coor, cr


_ANGLE_CRITERIA = {'MSELoss1D': 'mse', 'MSELoss': 'mse', 'SmoothL1Loss1D': 'sl1', 'SmoothL1Loss': 'sl1'}


def _angle_type(loss_func, cfgs):
    """'mse' / 'sl1' for the angle head: from the criterion object's class name, then from
    cfgs['heatmapModel']['loss_type'] (train_IGRs.py:42 evaluates that name in libs/loss/function.py)."""
    name = type(loss_func).__name__ if loss_func is not None else None
    if name in _ANGLE_CRITERIA:
        reduction = getattr(getattr(loss_func, 'criterion', loss_func), 'reduction', 'mean')
        if reduction != 'mean':
            raise NotImplementedError("%s(reduction=%r): the native angle step averages over the 2N elements "
                                      "('mean')" % (name, reduction))
        return _ANGLE_CRITERIA[name]
    cfg_name = cfgs.get('heatmapModel', {}).get('loss_type')
    if cfg_name in _ANGLE_CRITERIA:
        return _ANGLE_CRITERIA[cfg_name]
    raise NotImplementedError("the 'angleregression' head trains with MSELoss1D or SmoothL1Loss1D "
                              '(libs/loss/function.py:204-228); got loss_func %s and heatmapModel.loss_type %r'
                              % (name, cfg_name))


def integral_terms(cfgs):
    """cfgs['heatmapModel']['integral_terms']: train the heat-map head's coordinate and cross-ratio terms on the
    soft-arg-max of its maps (off when absent; YAML booleans, or the strings a hand-written file may hold)."""
    v = cfgs.get('heatmapModel', {}).get('integral_terms', False)
    if isinstance(v, str):
        if v.strip().lower() in ('true', 'yes', 'on', '1'):
            return True
        if v.strip().lower() in ('false', 'no', 'off', '0', 'none', ''):
            return False
        raise ValueError('heatmapModel.integral_terms must be a boolean, got %r' % (v,))
    return bool(v)


def make_step(model, cfgs, loss_func=None, optim=None):
    """The native step object for ``model`` (HC or L), configured like the reference's loss / optimizer."""
    lr = optim.param_groups[0]['lr'] if optim is not None else cfgs['optimizer']['lr']
    sync = parallel.FlatGradSync() if torch.distributed.is_available() and torch.distributed.is_initialized() \
        and torch.distributed.get_world_size() > 1 else None
    inner = model.module if hasattr(model, 'module') else model          # DataParallel / DDP wrappers
    # Parameter groups that differ (in their learning rate too), AdamW, AMSGrad, Nesterov, dampening or clipping go to
    # the grouped update as a spec (optim.py); everything the one-launch update can express goes the old way.
    max_grad_norm = _max_grad_norm(cfgs)
    if optim is not None and optim_spec.needs_grouped(optim, max_grad_norm):
        okw = dict(optim_spec=optim_spec.spec_from_torch(optim), max_grad_norm=max_grad_norm)
    else:
        okw = _optim_kwargs(optim, cfgs)
        if max_grad_norm is not None:
            okw['max_grad_norm'] = max_grad_norm
    if isinstance(inner, PoseHighResolutionNet) and inner.head_type == 'angleregression':
        step = HRNetTrainStep(inner, lr=lr, grad_sync=sync, angle_type=_angle_type(loss_func, cfgs),
                              **okw)
        step.apply_cr_loss = False
        return step
    if isinstance(inner, PoseHighResolutionNet):
        w_hm, w_coor, cr = _loss_weights(loss_func, cfgs)
        sigma = cfgs.get('heatmapModel', {}).get('sigma', 1)
        if inner.head_type == 'heatmap':
            # The reference switches the heat-map head's terms by loss_type (JointsMSELoss: the map term alone;
            # JointsCompositeLoss: L_2d and L_cr on the soft-arg-max as well, function.py:187-201).  Here the key
            # heatmapModel.integral_terms does: a criterion object alone changes nothing, so the heat-map runs that
            # exist keep their loss bit for bit.
            if not integral_terms(cfgs):
                w_coor, cr = 0.0, {k: v for k, v in cr.items() if k == 'hm_type'}
            # JointsMSELoss(use_target_weight=...) (tools/train_IGRs.py:42, function.py:22-46)
            cr['use_target_weight'] = bool(getattr(loss_func, 'use_target_weight',
                                                   cfgs.get('training_settings', {}).get('use_target_weight', False)))
        cr.update(okw)
        step = HRNetTrainStep(inner, lr=lr, w_hm=w_hm, w_coor=w_coor, grad_sync=sync, sigma=sigma, **cr)
        step.apply_cr_loss = bool(getattr(loss_func, 'apply_cr_loss', False))
        return step
    if isinstance(inner, FCmodel.FCModel):
        return LifterTrainStep(inner, lr=lr, grad_sync=sync, **okw)
    raise TypeError('no native training step for %s' % type(inner).__name__)


def _max_grad_norm(cfgs):
    """cfgs['optimizer']['max_grad_norm'] (absent / None / 'None': no clipping)."""
    v = (cfgs.get('optimizer') or {}).get('max_grad_norm')
    return None if v in (None, 'None', '') else float(v)


# -- training checkpoints (training_settings.checkpoint / checkpoint_every / resume) --------------------------------------
_FINGERPRINT_OPTIM_KEYS = ('optim_type', 'weight_decay', 'momentum', 'amsgrad', 'nesterov', 'dampening',
                           'no_decay_norm_bias', 'max_grad_norm')


def _world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _path_or_none(v):
    """A path key of training_settings: absent, None, False, '' and the strings 'False' / 'None' are off."""
    return None if v in (None, False, '', 'False', 'false', 'None') else str(v)


def _fingerprint(model, cfgs):
    inner = model.module if hasattr(model, 'module') else model
    o = cfgs.get('optimizer') or {}
    keys = {}
    for k in _FINGERPRINT_OPTIM_KEYS:
        v = o.get(k)
        keys[k] = v if v is None or isinstance(v, (bool, str)) else float(v)
    return {'exp_type': str(cfgs.get('exp_type')), 'head_type': str(getattr(inner, 'head_type', type(inner).__name__)),
            'optimizer': keys, 'world_size': _world()}


def rank_file(path, rank=None):
    """``<path>.rank<r>``: the per-rank part of a training checkpoint."""
    return '%s.rank%d' % (path, _rank() if rank is None else rank)


def _write(obj, path):
    tmp = path + '.tmp'
    torch.save(obj, tmp)
    os.replace(tmp, path)


def save_checkpoint(path, model, step, optim, sche, cfgs, epochs, x_buffer=(), y_buffer=()):
    """A training checkpoint after ``epochs`` completed epochs.  Rank 0 writes ``path`` (tmp + ``os.replace``): the
    model's ``state_dict()`` after ``parallel.broadcast_buffers``, the step's ``state_dict()``, ``optimizer`` -- the same
    state in ``torch.optim.Optimizer.state_dict()`` form, what a reference-style reader looks for --, the scheduler's
    ``state_dict()``, the torch optimizer's ``param_groups`` hyper-parameters, the loss history and a fingerprint of the
    configuration.  Every rank writes ``<path>.rank<r>`` itself: Python's, numpy's and torch's CPU and CUDA generator
    states and the lifter's dropout seed.  Then the barrier: nobody resumes from a file before it is complete.  Both
    files load with ``torch.load(..., weights_only=True)``.  ``optim`` (may be None) is read, never changed."""
    from . import train_state
    parallel.broadcast_buffers(model, src=0)
    rank_part = {'rank': _rank(), 'world_size': _world(), 'rng': train_state.rng_state(step.flat.flat.device),
                 'drop_seed': int(step.drop_seed) if hasattr(step, 'drop_seed') else None}
    _write(rank_part, rank_file(path))
    if _rank() == 0:       # one writer, like the snapshots
        inner = model.module if hasattr(model, 'module') else model
        groups = None if optim is None else [{k: v for k, v in g.items() if k != 'params'} for g in optim.param_groups]
        _write({'format': train_state.FORMAT, 'epochs': int(epochs),
                'model': {k: v.detach().cpu().clone() for k, v in inner.state_dict().items()},
                'step': step.state_dict(), 'optimizer': train_state.optimizer_state_dict(step),
                'scheduler': None if sche is None else sche.state_dict(), 'param_groups': groups,
                'batch_idx': [int(x) for x in x_buffer], 'loss': [float(y) for y in y_buffer],
                'fingerprint': _fingerprint(model, cfgs)}, path)
    _barrier()


def load_checkpoint(path, model, step, optim, sche, cfgs, total_epochs=None):
    """The inverse of ``save_checkpoint`` on freshly built objects: model, step, scheduler, the torch optimizer's
    ``param_groups`` hyper-parameters and this rank's generator states.  Returns the checkpoint's dict (``epochs``,
    ``batch_idx``, ``loss``, ...).  ``ValueError``, before anything is written, when the fingerprint or the world size
    differs, this rank's file is missing, or ``total_epochs`` is given and the run has already completed them."""
    from . import train_state
    if not os.path.isfile(path):
        raise ValueError('no training checkpoint at %s' % path)
    ck = torch.load(path, map_location='cpu', weights_only=True)
    if ck.get('format') != train_state.FORMAT:
        raise ValueError('training-checkpoint format %r (this version reads %d)' % (ck.get('format'), train_state.FORMAT))
    want, have = ck['fingerprint'], _fingerprint(model, cfgs)
    if want['world_size'] != have['world_size']:
        raise ValueError('the checkpoint was written by %d ranks, this run has %d' % (want['world_size'],
                                                                                    have['world_size']))
    for k in ('exp_type', 'head_type'):
        if want[k] != have[k]:
            raise ValueError('the checkpoint has %s %r, this run %r' % (k, want[k], have[k]))
    for k in _FINGERPRINT_OPTIM_KEYS:
        if want['optimizer'].get(k) != have['optimizer'].get(k):
            raise ValueError('the checkpoint has optimizer.%s %r, this run %r'
                             % (k, want['optimizer'].get(k), have['optimizer'].get(k)))
    mine = rank_file(path)
    if not os.path.isfile(mine):
        raise ValueError('the per-rank file %s is missing' % mine)
    if total_epochs is not None and ck['epochs'] >= total_epochs:
        raise ValueError('the checkpoint has completed %d epochs, total_epochs is %d: nothing left to run'
                         % (ck['epochs'], total_epochs))
    rank_part = torch.load(mine, map_location='cpu', weights_only=True)
    if rank_part['world_size'] != have['world_size'] or rank_part['rank'] != _rank():
        raise ValueError('%s was written by rank %d of %d' % (mine, rank_part['rank'], rank_part['world_size']))
    if optim is not None and ck.get('param_groups') is not None and len(ck['param_groups']) != len(optim.param_groups):
        raise ValueError('%d param_groups in the checkpoint, the optimizer has %d'
                         % (len(ck['param_groups']), len(optim.param_groups)))
    inner = model.module if hasattr(model, 'module') else model
    step.load_state_dict(ck['step'])                    # validates first: nothing is written when it refuses
    inner.load_state_dict(ck['model'])                  # in place: the parameters stay views of the flat buffer
    from .engine import invalidate
    invalidate(inner)
    if rank_part.get('drop_seed') is not None and hasattr(step, 'drop_seed'):
        step.drop_seed = int(rank_part['drop_seed'])    # this rank's own (the step state is rank 0's)
    if optim is not None and ck.get('param_groups') is not None:
        for g, saved in zip(optim.param_groups, ck['param_groups']):
            g.update(saved)
    if sche is not None and ck.get('scheduler') is not None:
        sche.load_state_dict(ck['scheduler'])
    train_state.set_rng_state(rank_part['rng'], step.flat.flat.device)
    return ck


class _Acc(object):
    """The reference's AverageMeter for the optional training metric (utils.py:149-182)."""

    def __init__(self):
        self.sum, self.count, self.others = 0.0, 0, None

    def update(self, val, n=1, others=None):
        self.sum += float(val) * n
        self.count += n
        self.others = others

    @property
    def avg(self):
        return self.sum / self.count if self.count else 0.0


def evaluate(eval_dataset, model, loss_func, cfgs, logger, evaluator, save=False, save_path=None,
             collate_fn=None, epoch=None, sample_num=20):
    """trainer.py:395-513.  ``model.eval()`` + ``model(data)`` per batch with autograd ENABLED, like
    the reference: for CUDA batches that is the HIP inference program (hrnet.py / FCmodel.py
    ``forward``).  ``loss_func`` (the caller's criterion, optional) and ``evaluator``
    (``update(prediction, ground_truth=, meta_data=)`` / ``report(logger)``) are called like the
    reference calls them; 3D plotting (``vis_epoch``) is outside the hot path and skipped.
    An evaluator with ``device_update = True`` (``metric.criterions.Evaluator`` over the lifter's 3-D metrics) gets
    the CUDA prediction / target as they are -- with ``testing_settings.unnormalize`` also the set's ``statistics``,
    its kernel unnormalises -- instead of the ``.cpu().numpy()`` copies and the host unnormalise.
    ``testing_settings.save_debug`` with ``exp_type == 'instanceto2d'`` writes the debug pictures of every batch like
    trainer.py:450-466 (epoch 0, split 'validation'; rank 0 only).
    Returns the mean validation loss (None without ``loss_func``)."""
    ts = cfgs['testing_settings']
    writer = debug_pictures.DebugPictureWriter() if ts.get('save_debug', False) and \
        cfgs.get('exp_type') == 'instanceto2d' and _rank() == 0 else None
    try:
        return _evaluate(eval_dataset, model, loss_func, cfgs, logger, evaluator, save, save_path, collate_fn, epoch,
                         writer)
    finally:
        if writer is not None:
            writer.close()


def _evaluate(eval_dataset, model, loss_func, cfgs, logger, evaluator, save, save_path, collate_fn, epoch, writer):
    ts = cfgs['testing_settings']
    unnorm = bool(ts.get('unnormalize', False))
    stats = eval_dataset.statistics if unnorm else None
    dev_eval = evaluator is not None and bool(getattr(evaluator, 'device_update', False))
    model.eval()
    if ts.get('apply_dropout', False):
        # trainer.py:424-428: dropout layers back in train mode ("a loss similar to the training loss"); the model's
        # forward sees that state and takes its torch graph (FCModel._dropout_active) -- the HIP program has no dropout
        def apply_dropout(m):
            if type(m) == torch.nn.Dropout:
                m.train()
        model.apply(apply_dropout)
    loader = get_loader(eval_dataset, cfgs, 'testing', collate_fn)
    use_cuda = cfgs.get('use_gpu', True) and torch.cuda.is_available()
    loss_sum, seen = 0.0, 0
    preds, gts = [], []
    for batch_idx, (data, target, weights, meta) in enumerate(loader):
        if use_cuda:
            data, target = data.cuda(), target.cuda()
            weights = weights.cuda() if torch.is_tensor(weights) else weights
        prediction = model(data)
        if writer is not None:
            debug_pictures.save_debug_images(0, batch_idx, cfgs, data, meta, target, None, prediction, 'validation',
                                             writer=writer)
            logger.info('Saved batch {:d}'.format(batch_idx))
        if loss_func is not None:
            with torch.no_grad():
                loss = loss_func(prediction, target, weights, meta)
            loss_sum += float(loss.item()) * data.size(0)
            seen += data.size(0)
        fused = unnorm and dev_eval and torch.is_tensor(prediction) and prediction.is_cuda
        if fused:                                   # both stay in HBM: the evaluator's kernel unnormalises
            evaluator.update(prediction, ground_truth=target, meta_data=meta, statistics=stats)
            if save:
                target = eval_dataset.unnormalize(target.data.cpu().numpy(), stats['mean_out'], stats['std_out'])
                prediction = eval_dataset.unnormalize(prediction.data.cpu().numpy(), stats['mean_out'],
                                                      stats['std_out'])
        elif unnorm:
            target = eval_dataset.unnormalize(target.data.cpu().numpy(), stats['mean_out'], stats['std_out'])
            prediction = eval_dataset.unnormalize(prediction.data.cpu().numpy(), stats['mean_out'], stats['std_out'])
        if evaluator is not None and not fused:
            evaluator.update(prediction, ground_truth=target, meta_data=meta)
        if save:
            preds.append(prediction if isinstance(prediction, np.ndarray) else
                         (prediction[0] if isinstance(prediction, tuple) else prediction).data.cpu().numpy())
            gts.append(target if isinstance(target, np.ndarray) else target.data.cpu().numpy())
    if save:
        np.save(save_path, np.array({'pred': np.concatenate(preds, axis=0), 'error': [],
                                     'gt': np.concatenate(gts, axis=0)}, dtype=object))
    if evaluator is not None:
        evaluator.report(logger)
    mean_loss = loss_sum / seen if seen else None
    if mean_loss is not None:
        logger.info('Validation%s: loss %.6f over %d samples' % (
            '' if epoch is None else ' (epoch %d)' % epoch, mean_loss, seen))
    return mean_loss


def train(train_dataset, model, loss_func, optim, sche, cfgs, logger, metric_func=None, stats=None,
          valid_dataset=None, collate_fn=None, save_debug=False, evaluate_fn=None, evaluator=None,
          sample_builder=None):
    """trainer.py:127-263.  Validation during training (``eval_during``): ``evaluate_fn(valid_dataset,
    model, epoch)`` if given, else this module's ``evaluate`` with ``evaluator``; with neither, an
    ``Evaluator(training_settings.eval_metrics, cfgs, train_dataset.num_joints)`` is built like the reference's
    (trainer.py:151-156) -- one object for the whole run, so its statistics run over every validation pass, as there.
    ``metric_func``: a callable ``(prediction, meta, cfgs) -> (avg, cnt, others)`` run on every batch, or an object
    with ``accumulate(prediction, meta, cfgs)`` / ``read() -> (running mean, count, ...)`` / ``reset()``
    (``metric.criterions.DistanceSrcMeter``): accumulated on every batch without a read-back, reset at the start of an
    epoch, read only on report batches.
    ``sample_builder``: a callable (``common.train_samples.TrainSampleBuilder``) that turns each loader item
    -- e.g. the list of decoded frame records ``common.train_samples.collate_frames`` yields -- into the
    ``(data, target, weights, meta)`` batch; None: the loader yields that batch itself.
    A mixed batch (``cfgs['ss']``, car_instance.py:1368-1380) passes through as it is: ``data`` holds ``N`` crops, the
    labelled ones first, ``target`` and ``meta['transformed_joints']`` their ``n_fs <= N`` rows; the step takes the
    heat-map and coordinate terms over the labelled prefix and the cross-ratio term over all crops, a metric sees the
    ``N`` predictions and the ``n_fs`` meta rows, and the logged samples/s counts ``N``.
    ``save_debug``: on report batches, where the loss is read back, the reference's three debug pictures
    (``visualization.debug.save_debug_images``, gated by ``training_settings.debug``) are composed on the device and
    handed to a ``DebugPictureWriter``, closed when the loop ends; heat-map and coordinate heads on rank 0 only -- the
    angle head and the lifter have no maps and skip silently.  Off (the default), no writer is made and the step's
    launches are unchanged.
    ``training_settings.checkpoint`` (a path; ``checkpoint_every`` epochs, default 1) writes a training checkpoint at
    the end of an epoch (``save_checkpoint``); ``training_settings.resume`` (a path, or False: the reference's key)
    loads one into the freshly built step, model, scheduler and optimizer groups and continues with the epoch after its
    last (``load_checkpoint``, which refuses with ValueError before any step runs); the record then holds the whole
    run's loss history.  All three absent or false (the default): nothing differs."""
    ts = cfgs['training_settings']
    total_epochs, report_every = ts['total_epochs'], ts['report_every']
    eval_during = bool(ts.get('eval_during', False)) and valid_dataset is not None
    if eval_during and evaluate_fn is None and evaluator is None and ts.get('eval_metrics'):
        from .metric.criterions import Evaluator
        evaluator = Evaluator(ts['eval_metrics'], cfgs, train_dataset.num_joints)
    if eval_during and evaluate_fn is None and evaluator is None:
        logger.warning('training_settings.eval_during is set but neither evaluate_fn nor evaluator was given: '
                       'no validation during training')
        eval_during = False
    if eval_during and evaluate_fn is None:
        def evaluate_fn(ds, mdl, ep):
            return evaluate(ds, mdl, loss_func if callable(loss_func) else None, cfgs, logger, evaluator,
                            collate_fn=collate_fn, epoch=ep)
    eval_every = ts.get('eval_every', 0)
    eval_start = ts.get('eval_start_epoch', 0)
    step = make_step(model, cfgs, loss_func, optim)
    is_hc = isinstance(step, HRNetTrainStep)
    is_angle = is_hc and step.angle_crit is not None           # baselinealpha / baselinetheta: one term, no L_cr
    maps_only = getattr(model.module if hasattr(model, 'module') else model, 'head_type', None) == 'heatmap'
    dev = step.dev
    # a metric with accumulate / read / reset (metric.criterions.DistanceSrcMeter) keeps its running sums on the device
    metric_on_device = metric_func is not None and hasattr(metric_func, 'accumulate')
    x_buffer, y_buffer = [], []
    # training checkpoints: all three keys absent or false by default, and then nothing below differs from a run
    # without them
    ckpt_path, resume = _path_or_none(ts.get('checkpoint')), _path_or_none(ts.get('resume'))
    ckpt_every = max(int(ts.get('checkpoint_every') or 1), 1)
    first_epoch = 1
    if resume is not None:
        ck = load_checkpoint(resume, model, step, optim, sche, cfgs, total_epochs=total_epochs)
        first_epoch = ck['epochs'] + 1
        x_buffer, y_buffer = list(ck['batch_idx']), list(ck['loss'])
        logger.info('=> Resumed from %s: %d epochs completed, starting at epoch %d' % (resume, ck['epochs'], first_epoch))
        del ck
    frozen = False
    writer = debug_pictures.DebugPictureWriter() if save_debug and is_hc and not is_angle and _rank() == 0 else None
    if eval_during:
        _make_host_group()      # all ranks are here together: the group exists before anyone has to wait in it
    try:
        for epoch in range(first_epoch, total_epochs + 1):
            if epoch > 1 and is_hc and not is_angle:
                step.apply_cr_loss = True                       # trainer.py:168-169: L_cr from the second epoch on
            model.train()
            if sche is not None:
                sche.step()                                     # trainer.py:177, before the epoch like the reference
            if optim is not None:
                step.set_lrs([g['lr'] for g in optim.param_groups])      # every group's, not the first alone
            loader = get_loader(train_dataset, cfgs, 'training', collate_fn)
            total_batches, t_epoch = len(loader), time.time()
            acc = _Acc()
            if metric_on_device:
                metric_func.reset()
            for batch_idx, batch in enumerate(loader):
                if sample_builder is not None:
                    batch = sample_builder(batch)
                data, target, weights, meta = batch
                data = data.to(dev, non_blocking=True)
                target = target.to(dev, non_blocking=True)
                if is_angle:
                    loss = step.step(data, target)
                    prediction = step.last_angles
                elif is_hc:
                    joints = meta['transformed_joints'] if step.w_coor else None
                    loss = step.step(data, target, joints,
                                     target_weight=weights if step.use_target_weight else None)
                    # (the heat-map head's output is its maps, also when its integral terms fill last_coords)
                    prediction = (step.last_maps, step.last_coords) \
                        if step.last_coords is not None and not maps_only else step.last_maps
                else:
                    loss = step.step(data, target)
                    prediction = None
                # the optional metric runs on EVERY batch and accumulates, like the reference
                # (trainer.py:200-205); a plain callable decodes on the device and returns a host number, a meter
                # only launches and is read back where the loss is
                others = None
                if metric_func is not None and prediction is not None:
                    if metric_on_device:
                        metric_func.accumulate(prediction, meta, cfgs)
                    else:
                        avg_acc, cnt, others = metric_func(prediction, meta, cfgs)
                        acc.update(avg_acc, n=cnt, others=others)
                if not frozen:
                    # everything built so far (model, datasets, the step's packed filters, torch's module
                    # tables: millions of objects) moves to the permanent generation: the full collections
                    # the per-iteration Python objects trigger every ~10 iterations then take < 1 ms
                    # instead of 35 ms of a host that has 1 500 launches per iteration to issue
                    gc.collect()
                    gc.freeze()
                    frozen = True
                if batch_idx % report_every == 0:               # loss read-back only here
                    lv = float(loss.item())
                    logger.info('Epoch: [%d][%d/%d]  loss %.6f  lr %.2e  %.1f samples/s' % (
                        epoch, batch_idx, total_batches, lv, step.lr,
                        (batch_idx + 1) * data.size(0) / max(time.time() - t_epoch, 1e-9)))
                    if metric_on_device and prediction is not None:
                        run_mean, run_cnt = metric_func.read()[:2]         # the meter's one read-back
                        if run_cnt:
                            logger.info('          metric %.6f (running mean over %d)' % (run_mean, run_cnt))
                    elif acc.count:
                        logger.info('          metric %.6f (running mean over %d)' % (acc.avg, acc.count))
                    if writer is not None:
                        debug_pictures.save_debug_images(epoch, batch_idx, cfgs, data, meta, target, others, prediction,
                                                         'train', writer=writer)
                    x_buffer.append(total_batches * (epoch - 1) + batch_idx)
                    y_buffer.append(lv)
                if eval_during and epoch > eval_start and batch_idx and eval_every and batch_idx % eval_every == 0:
                    parallel.broadcast_buffers(model, src=0)    # running statistics follow rank 0 (DataParallel semantics)
                    # every rank holds the same weights and (now) buffers: rank 0 evaluates the validation set
                    # (ts['eval_all_ranks'] restores one evaluation per rank), the others wait for it.
                    # CONTRACT: unless 'eval_all_ranks' is set, `evaluate_fn` runs on rank 0 ONLY -- it must
                    # not contain collectives or DistributedSampler logic (they would wait for ranks that never call
                    # them).  The waiting ranks block in a barrier of a HOST-side gloo group made at the start of
                    # train() (12 h timeout), not on a GPU barrier kernel; if that group could not be made, in the
                    # default group's barrier (bounded by ITS timeout: choose `timeout=` in init_process_group).
                    if _rank() == 0 or ts.get('eval_all_ranks', False):
                        evaluate_fn(valid_dataset, model, epoch)
                    _wait_for_rank0()
                    model.train()
            if epoch in ts.get('snapshot_epochs', []):
                parallel.broadcast_buffers(model, src=0)
                out_dir = cfgs.get('dirs', {}).get('output', '.')
                path = os.path.join(out_dir, '%s_%d.pth' % (cfgs.get('exp_type', 'model'), epoch))
                if _rank() == 0:       # one writer: concurrent truncating writers can leave a torn checkpoint
                    logger.info('=> Snapshot model to {}'.format(path))
                    inner = model.module if hasattr(model, 'module') else model
                    tmp = path + '.tmp'
                    torch.save(inner.state_dict(), tmp)
                    os.replace(tmp, path)
                _barrier()             # nobody reads / resumes from the file before it is complete
            if ckpt_path is not None and (epoch % ckpt_every == 0 or epoch == total_epochs):
                logger.info('=> Training checkpoint after epoch {:d} to {}'.format(epoch, ckpt_path))
                save_checkpoint(ckpt_path, model, step, optim, sche, cfgs, epoch, x_buffer, y_buffer)
    finally:
        if frozen:
            gc.unfreeze()
        if writer is not None:
            writer.close()
    logger.info('Training finished.')
    return {'model': model, 'batch_idx': x_buffer, 'loss': y_buffer}


def train_cascade(train_dataset, valid_dataset, cfgs, logger):
    """trainer.py:25-71: the lifter sub-model(s) L.pth, one stage after the other."""
    cascade = FCmodel.get_cascade()
    stage_record = []
    for stage_id in range(cfgs['cascade']['num_stages']):
        input_size, output_size = train_dataset.get_input_output_size()
        cfgs['FCModel']['input_size'] = input_size
        cfgs['FCModel']['output_size'] = output_size
        stage_model = FCmodel.get_fc_model(stage_id + 1, cfgs=cfgs, input_size=input_size, output_size=output_size)
        if not cfgs.get('use_gpu', True):
            raise ValueError('native training runs on the GPU (use_gpu: true)')
        stage_model = stage_model.cuda()
        optim, sche = prepare_optim(stage_model, cfgs)
        record = train(train_dataset=train_dataset, valid_dataset=valid_dataset, model=stage_model, loss_func=None,
                       optim=optim, sche=sche, stats=None, cfgs=cfgs, logger=logger)
        stage_record.append((record['batch_idx'], record['loss']))
        cascade.append(record['model'].cpu())
    return {'cascade': cascade, 'record': stage_record}
