"""VoiceBoxTrainer-compatible driver over the native data-parallel step.

Mirrors voicebox_pytorch/trainer.py:60-321: the dataset yields latents (frames, dim) or, for a model built with
audio_enc_dec, waves (samples,) that the codec encodes inside the step; same constructor keywords, `train_step` / `train` / `save` / `load`, the same learning-rate rule (linear warm-up,
then one CosineAnnealingLR step per training step, :231-253), gradient accumulation with a deferred exchange (= accelerator.no_sync
on all but the last micro-batch, :258-272), global-norm clipping (:274-275), Adam(betas=(0.9, 0.99)) (optimizer.py:10-35), rank-0
validation and checkpoints in the reference's format `{'model', 'optim', 'scheduler'}` (:191-197) -- `optim` is a
torch.optim.Adam state_dict over `cfm_wrapper.parameters()` order, so checkpoints interchange with the reference trainer.

No Accelerate: one process per GPU with torch.distributed already initialised by the launcher (or a single process).
"""
import re
from pathlib import Path
from shutil import rmtree

import torch
import torch.distributed as dist
from torch import nn
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import DataLoader, Dataset, random_split

from .dp import TrainStep, WarmupCosineLR
from .model import ConditionalFlowMatcherWrapper


def exists(v):
    return v is not None


def cycle(dl, sampler=None):
    epoch = 0
    while True:
        if sampler is not None:  # DistributedSampler reshuffles only when told the epoch (accelerate's prepared loader does this)
            sampler.set_epoch(epoch)
        for data in dl:
            yield data
        epoch += 1


def checkpoint_num_steps(checkpoint_path):  # trainer.py:44-57
    results = re.findall(r'\d+', str(checkpoint_path))
    return int(results[-1]) if len(results) else 0


def _collate(pad_to_longest, with_lens=False):  # data.py:69-101 (tensors only)
    """with_lens (VoiceBoxTrainer(mask_padding=True)): the batch tuple gets one more entry behind the padded columns -- the length of
    each item of the FIRST column before pad_sequence (int64 [B]; the cropped length without pad_to_longest)."""
    def one(data):
        if pad_to_longest:
            return pad_sequence(list(data), batch_first=True)
        n = min(d.shape[0] for d in data)
        return torch.stack([d[:n] for d in data])

    def inner(batch):
        if not isinstance(batch[0], tuple):
            return (one(batch),)
        return tuple(one(col) for col in zip(*batch))

    def inner_lens(batch):
        out = inner(batch)
        first = batch if not isinstance(batch[0], tuple) else [item[0] for item in batch]
        return out + (torch.tensor([min(d.shape[0], out[0].shape[1]) for d in first], dtype=torch.int64),)

    return inner_lens if with_lens else inner


def get_dataloader(ds, pad_to_longest=True, with_lens=False, **kwargs):  # data.py:103-105
    return DataLoader(ds, collate_fn=_collate(pad_to_longest, with_lens), **kwargs)


def _adapter_moments(ts):
    """{id(adapter parameter): (exp_avg view, exp_avg_sq view)} of the LoRA adapters a TrainStep trains (empty without adapters)."""
    if not hasattr(ts, "_refresh_trainable"):
        return {}
    ts._refresh_trainable()
    lo = getattr(ts, "_lora_rt", None)
    out = {}
    if lo is not None:
        for e in lo["state"].entries:
            for p, off in ((e["module"].lora_A, e["a_off"]), (e["module"].lora_B, e["b_off"])):
                out[id(p)] = (lo["m"][off:off + p.numel()].view(p.shape), lo["v"][off:off + p.numel()].view(p.shape))
    return out


class VoiceBoxTrainer(nn.Module):
    def __init__(self, cfm_wrapper: ConditionalFlowMatcherWrapper, *, batch_size, dataset: Dataset, num_train_steps=None,
                 num_warmup_steps=None, num_epochs=None, lr=3e-4, initial_lr=1e-5, grad_accum_every=1, wd=0., max_grad_norm=0.5,
                 valid_frac=0.05, random_split_seed=42, log_every=10, save_results_every=100, save_model_every=1000,
                 results_folder='./results', force_clear_prev_results=None, split_batches=False, drop_last=False,
                 accelerate_kwargs: dict = dict(), length_bucket=64, input_sampling_rate=None, mask_padding=False,
                 mask_wave_padding=False,
                 ema_decay=None, ema_update_after_step=0, ema_inv_gamma=1.0, ema_power=None):
        # length_bucket (not a reference keyword): batches of a varying-length dataset are padded with masked frames to the next
        # multiple of it, so that training runs on a handful of activation arenas (dp.TrainStep); 0 = exact lengths
        # input_sampling_rate (not a reference keyword: its trainer never passes one): the rate of a dataset of waves, handed to
        # every train and validation step; a wrapper built with resample_input=True resamples them to the codec's rate
        # mask_padding (not a reference keyword; opt-in, because the reference trains on the frames pad_sequence adds): the collate
        # function also returns each item's length, and every train and validation step passes lens= -- padding frames are masked in the
        # convolution, the attention and the loss, and the attention kernels stop at each row's length.  Latent datasets only: with a
        # dataset of waves the first batch raises ValueError (the frame count is the codec's business).
        # mask_wave_padding (not a reference keyword; opt-in): the same for a dataset of WAVES -- the collate function's lengths are samples
        # per row and go to every train and validation step as wave_lens=: every row is encoded as the row alone and its padding
        # frames are masked (wave_lens.py).  With a dataset of latents the first batch raises ValueError naming mask_padding.
        # ema_decay / ema_update_after_step / ema_inv_gamma / ema_power (not reference keywords): handed to dp.TrainStep, which keeps an
        # exponential moving average of the weights inside its Adam launches.  save() then adds 'ema_model' (TrainStep.ema_state_dict())
        # and 'ema' (the four hyper-parameters) beside the reference's three keys, load() restores the average from them (or resets it
        # to the loaded weights when the file has none), and the rank-0 validation also logs the loss of the averaged model.
        super().__init__()
        self.mask_padding = bool(mask_padding)
        self.mask_wave_padding = bool(mask_wave_padding)
        if self.mask_padding and self.mask_wave_padding:
            raise ValueError("VoiceBoxTrainer: mask_padding (a dataset of latents, lengths in frames) and mask_wave_padding (a dataset of "
                             "waves, lengths in samples) both given -- pass one of them")
        self.input_sampling_rate = input_sampling_rate
        assert isinstance(cfm_wrapper, ConditionalFlowMatcherWrapper)
        self.wd = float(wd)  # > 0: AdamW with decay on the ndim >= 2 parameters (get_optimizer, optimizer.py:10-35)
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank = dist.get_rank() if self.distributed else 0
        self.world = dist.get_world_size() if self.distributed else 1
        # split_batches (trainer.py:83,93 -> Accelerator(split_batches=...)): batch_size is the GLOBAL batch of a step, every rank
        # loads batch_size / world of it (False, Accelerate's default: every rank loads its own batch_size samples)
        self.split_batches = bool(split_batches)
        self.rank_batch_size = self.rank_batch(batch_size, self.world, self.split_batches)
        self.cfm_wrapper = cfm_wrapper
        self.register_buffer('steps', torch.Tensor([0]))
        self.batch_size, self.grad_accum_every = batch_size, grad_accum_every
        self.lr, self.initial_lr, self.max_grad_norm = lr, initial_lr, max_grad_norm

        self.ds = dataset
        if valid_frac > 0:  # trainer.py:121-131
            train_size = int((1 - valid_frac) * len(self.ds))
            valid_size = len(self.ds) - train_size
            self.ds, self.valid_ds = random_split(self.ds, [train_size, valid_size],
                                                  generator=torch.Generator().manual_seed(random_split_seed))
            self.print(f'training with dataset of {len(self.ds)} samples and validating with randomly splitted {len(self.valid_ds)} samples')
        else:
            self.valid_ds = self.ds
            self.print(f'training with shared training and valid dataset of {len(self.ds)} samples')
        assert len(self.ds) >= batch_size, 'dataset must have sufficient samples for training'
        assert len(self.valid_ds) >= batch_size, \
            f'validation dataset must have sufficient number of samples (currently {len(self.valid_ds)}) for training'
        assert exists(num_train_steps) or exists(num_epochs), 'either num_train_steps or num_epochs must be specified'
        self.num_train_steps = len(dataset) // batch_size * num_epochs if exists(num_epochs) else num_train_steps
        self.num_warmup_steps = num_warmup_steps if exists(num_warmup_steps) else 0
        self.schedule = WarmupCosineLR(lr, self.num_train_steps, self.num_warmup_steps, initial_lr)
        self.train_step_fn = TrainStep(cfm_wrapper, lr=lr, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=max_grad_norm, wd=self.wd,
                                       lr_schedule=None, length_bucket=length_bucket, ema_decay=ema_decay,
                                       ema_update_after_step=ema_update_after_step, ema_inv_gamma=ema_inv_gamma, ema_power=ema_power)

        sampler = None
        if self.world > 1:  # what accelerator.prepare(dl) does: each rank sees its own shard
            sampler = torch.utils.data.distributed.DistributedSampler(self.ds, num_replicas=self.world, rank=self.rank, shuffle=True)
        self.dl = get_dataloader(self.ds, batch_size=self.rank_batch_size, shuffle=sampler is None, sampler=sampler, drop_last=drop_last,
                                 with_lens=self.mask_padding or self.mask_wave_padding)
        self.valid_dl = get_dataloader(self.valid_ds, batch_size=batch_size, shuffle=True, drop_last=drop_last,
                                       with_lens=self.mask_padding or self.mask_wave_padding)
        self.dl_iter, self.valid_dl_iter = cycle(self.dl, sampler), cycle(self.valid_dl)
        self.log_every, self.save_model_every, self.save_results_every = log_every, save_model_every, save_results_every
        self.results_folder = Path(results_folder)
        if self.is_main and force_clear_prev_results is True and self.results_folder.exists():
            rmtree(str(self.results_folder))
        self.results_folder.mkdir(parents=True, exist_ok=True)

    @staticmethod
    def rank_batch(batch_size, world, split_batches):
        """Samples one rank loads per step: batch_size (Accelerate's default) or batch_size / world (split_batches=True)."""
        if not split_batches:
            return batch_size
        if batch_size % world:
            raise ValueError(f"split_batches=True: batch_size ({batch_size}) must be a round multiple of the number of processes "
                             f"({world})")  # Accelerate's own condition
        return batch_size // world

    # ---- checkpoint format of the reference (trainer.py:191-207)
    def _optim_param_order(self):
        """Parameters in the order the reference's optimizer holds them: cfm_wrapper.parameters(), or -- with weight decay -- the
        ndim >= 2 parameters followed by the others (the two param groups get_optimizer builds, optimizer.py:4-9,24-30)."""
        params = list(self.cfm_wrapper.parameters())
        if self.wd > 0:
            wd_p = [p for p in params if p.ndim >= 2]
            return wd_p + [p for p in params if p.ndim < 2], len(wd_p)
        return params, len(params)

    def _optim_state_dict(self, gathered=False):
        ts = self.train_step_fn
        if not gathered:
            # grad_mode="shard": the moments of a chunk live on its owner; gathering them is a collective, so a direct save() /
            # _optim_state_dict() call must be made by EVERY rank (train_step() gathers on all ranks itself and passes gathered=True)
            ts.gather_optimizer_state()
        fp = ts.fp
        by_param = {id(fp.slots[s]): s for s in fp.order}
        state = {}
        params, n_wd = self._optim_param_order()
        adapters = _adapter_moments(self.train_step_fn)
        for i, p in enumerate(params):
            s = by_param.get(id(p))
            if s is None and id(p) in adapters and ts.steps > 0:  # a LoRA adapter: its moments live beside the adapter buffer
                state[i] = {'step': torch.tensor(float(ts.steps)), 'exp_avg': adapters[id(p)][0].clone(),
                            'exp_avg_sq': adapters[id(p)][1].clone()}
                continue
            if s is None or ts.steps == 0:
                continue  # parameters that never received a gradient (null_cond) have no Adam state, as in torch
            o, n = fp.offsets[s], p.numel()
            state[i] = {'step': torch.tensor(float(ts.steps)), 'exp_avg': ts.m[o:o + n].view(p.shape).clone(),
                        'exp_avg_sq': ts.v[o:o + n].view(p.shape).clone()}
        base = dict(lr=self.schedule.cur, betas=tuple(ts.betas), eps=ts.eps, amsgrad=False, maximize=False, foreach=None,
                    capturable=False, differentiable=False, fused=None)
        if self.wd > 0:
            groups = [dict(base, weight_decay=self.wd, params=list(range(n_wd))),
                      dict(base, weight_decay=0, params=list(range(n_wd, len(params))))]
        else:
            groups = [dict(base, weight_decay=0, params=list(range(len(params))))]
        return {'state': state, 'param_groups': groups}

    def _load_optim_state_dict(self, sd):
        ts = self.train_step_fn
        fp = ts.fp
        by_param = {id(fp.slots[s]): s for s in fp.order}
        steps = 0
        params, n_wd = self._optim_param_order()
        # Validate BEFORE copying anything: a checkpoint saved under the other weight-decay grouping (a reference wd = 0
        # checkpoint into a wd > 0 trainer, or the reverse) numbers its parameters differently; torch.optim.load_state_dict raises a
        # ValueError here, and so do we -- a partial, silently mis-assigned Adam state is never left behind.
        want = [n_wd, len(params) - n_wd] if self.wd > 0 else [len(params)]
        got = [len(g['params']) for g in sd['param_groups']]
        if got != want:
            raise ValueError(f"loaded state dict has parameter groups of sizes {got}, this trainer (wd = {self.wd}) has {want}")
        for i, p in enumerate(params):
            st = sd['state'].get(i)
            if st is not None and (tuple(st['exp_avg'].shape) != tuple(p.shape) or tuple(st['exp_avg_sq'].shape) != tuple(p.shape)):
                raise ValueError(f"optimizer state {i} has shape {tuple(st['exp_avg'].shape)}, parameter has {tuple(p.shape)}")
        adapters = _adapter_moments(self.train_step_fn)
        for i, p in enumerate(params):
            st = sd['state'].get(i)
            s = by_param.get(id(p))
            if st is not None and s is None and id(p) in adapters:
                adapters[id(p)][0].copy_(st['exp_avg'])
                adapters[id(p)][1].copy_(st['exp_avg_sq'])
                steps = max(steps, int(float(st['step'])))
                continue
            if st is None or s is None:
                continue
            o, n = fp.offsets[s], p.numel()
            ts.m[o:o + n].copy_(st['exp_avg'].reshape(-1))
            ts.v[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
            steps = max(steps, int(float(st['step'])))
        ts.steps = steps

    def _scheduler_state_dict(self):  # loadable by torch's CosineAnnealingLR.load_state_dict
        sc = self.schedule
        return dict(T_max=sc.T, eta_min=0, base_lrs=[sc.lr], last_epoch=sc.sched_epoch, _step_count=sc.sched_epoch + 1,
                    _get_lr_called_within_step=False, _last_lr=[sc.cur], verbose=False)

    def save(self, path, gathered=False):
        """Reference checkpoint format.  With TrainStep(grad_mode="shard") and world size > 1 call it on EVERY rank (only rank 0 needs
        to pass a real path to keep) unless the optimizer state was gathered collectively beforehand (gathered=True)."""
        pkg = dict(model=self.cfm_wrapper.state_dict(), optim=self._optim_state_dict(gathered), scheduler=self._scheduler_state_dict())
        ts = self.train_step_fn
        if ts.ema is not None:  # two more keys; the reference's loader reads 'model' only, so the file still loads there
            pkg['ema_model'] = ts.ema_state_dict()
            pkg['ema'] = dict(ts.ema_hyper)
        torch.save(pkg, path)

    def load(self, path):
        pkg = self.cfm_wrapper.load(path)
        self.train_step_fn.fp = self.cfm_wrapper.voicebox.flat_params()  # load_state_dict copied into the flat views
        self.train_step_fn._dirty()
        self._load_optim_state_dict(pkg['optim'])
        ts = self.train_step_fn
        if ts.ema is not None:  # (a file written with EMA loads into a trainer without it: the extra keys are ignored)
            ts.ema_reset()  # the loaded weights; then the file's average over it, when it has one
            if 'ema_model' in pkg:
                ts.load_ema_state_dict(pkg['ema_model'])
        sc = pkg['scheduler']
        self.schedule.sched_epoch, self.schedule.cur = int(sc['last_epoch']), float(sc['_last_lr'][0])
        # + 1 to start from the next step and avoid overwriting the last checkpoint (trainer.py:206-207)
        self.steps = torch.tensor([checkpoint_num_steps(path) + 1], device=self.steps.device)

    def print(self, msg):
        if self.rank == 0:
            print(msg, flush=True)

    @property
    def device(self):
        return self.cfm_wrapper.device

    @property
    def is_distributed(self):
        return self.world > 1

    @property
    def is_main(self):
        return self.rank == 0

    def warmup(self, step):  # trainer.py:231-235
        if step < self.num_warmup_steps:
            return self.initial_lr + (self.lr - self.initial_lr) * step / self.num_warmup_steps
        return self.lr

    def _model_kwargs(self, batch):
        """(latents or waves,) or (latents or waves, cond_token_ids): the second column feeds a text-conditioned model as semantic ids."""
        x = batch[0]
        kw = dict(input_sampling_rate=self.input_sampling_rate) if exists(self.input_sampling_rate) else {}
        if getattr(self, "mask_padding", False):  # the collate function's last entry: the items' lengths before padding
            batch, lens = batch[:-1], batch[-1]
            if x.ndim == 2 or (x.ndim == 3 and x.shape[1] == 1):
                raise ValueError("VoiceBoxTrainer(mask_padding=True) needs a dataset of latents (frames, dim): the lengths of waves are "
                                 "in samples, and the frame count is the codec's business -- encode the dataset first, or leave "
                                 "mask_padding off")
            kw['lens'] = lens
        elif getattr(self, "mask_wave_padding", False):  # the same entry, counting samples
            batch, lens = batch[:-1], batch[-1]
            if not (x.ndim == 2 or (x.ndim == 3 and x.shape[1] == 1)):
                raise ValueError("VoiceBoxTrainer(mask_wave_padding=True) needs a dataset of waves (samples,): the lengths of latents are "
                                 "in frames -- pass mask_padding=True for them")
            kw['wave_lens'] = lens
        if len(batch) > 1 and self.cfm_wrapper.condition_on_text:
            kw['cond_token_ids'] = batch[1]
        return x, kw

    def train_step(self):  # trainer.py:237-313
        steps = int(self.steps.item())
        lr = self.schedule.rate_for_step(steps)
        ts = self.train_step_fn
        logs = {}
        if self.grad_accum_every == 1:
            x, kw = self._model_kwargs(next(self.dl_iter))
            loss = ts.step(x, lr=lr, **kw)
            logs['loss'] = float(loss)
        else:
            total = 0.
            for i in range(self.grad_accum_every):
                x, kw = self._model_kwargs(next(self.dl_iter))
                if i + 1 < self.grad_accum_every:   # accelerator.no_sync: no exchange (trainer.py:258-272)
                    loss = ts.accumulate(x, 1.0 / self.grad_accum_every, **kw)
                else:                              # last micro-batch: exchange overlapped with ITS backward, then clip + Adam
                    loss = ts.accumulate_last_and_apply(x, 1.0 / self.grad_accum_every, lr=lr, **kw)
                total += float(loss) / self.grad_accum_every
            logs['loss'] = total
        if not steps % self.log_every:
            self.print(f"{steps}: loss: {logs['loss']:0.3f}")
        if self.distributed:
            dist.barrier()
        if self.is_main and not (steps % self.save_results_every):  # rank-0 validation (:289-301)
            x, kw = self._model_kwargs(next(self.valid_dl_iter))
            dev = torch.device(self.device)
            if ts.ema is not None:  # the generator states the validation starts from: the averaged model gets the same draws below
                rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None)
            with torch.inference_mode():
                self.cfm_wrapper.eval()
                ids = kw.get('cond_token_ids')
                valid_loss = self.cfm_wrapper(x.to(self.device), input_sampling_rate=self.input_sampling_rate,
                                              **{k: kw[k] for k in ('lens', 'wave_lens') if k in kw},
                                              **({'semantic_token_ids': ids.to(self.device)} if ids is not None else {}))
            self.print(f'{steps}: valid loss {float(valid_loss):0.3f}')
            logs['valid_loss'] = float(valid_loss)
            if ts.ema is not None:
                # the same batch and the same random draws through the averaged weights, inside a forked generator state: the
                # training that follows draws what a trainer without EMA draws
                with torch.random.fork_rng(devices=[dev] if dev.type == 'cuda' else []), ts.ema_weights(), torch.inference_mode():
                    torch.set_rng_state(rng[0])
                    if rng[1] is not None:
                        torch.cuda.set_rng_state(rng[1], dev)
                    valid_loss_ema = self.cfm_wrapper(x.to(self.device), input_sampling_rate=self.input_sampling_rate,
                                                      **{k: kw[k] for k in ('lens', 'wave_lens') if k in kw},
                                                      **({'semantic_token_ids': ids.to(self.device)} if ids is not None else {}))
                self.print(f'{steps}: valid loss (ema) {float(valid_loss_ema):0.3f}')
                logs['valid_loss_ema'] = float(valid_loss_ema)
        if not (steps % self.save_model_every):
            # grad_mode="shard": the Adam moments of a chunk live on its owner -- collecting them is a COLLECTIVE, so every rank takes
            # part here, before rank 0 alone writes the file (a rank-0-only gather would hang or pair with the other ranks'
            # next-step collectives).  A no-op in all-reduce mode.
            self.train_step_fn.gather_optimizer_state()
        if self.is_main and not (steps % self.save_model_every):
            self.save(str(self.results_folder / f'voicebox.{steps}.pt'), gathered=True)
            self.print(f'{steps}: saving model to {str(self.results_folder)}')
        self.steps += 1
        return logs

    def train(self, log_fn=lambda logs: None):
        while self.steps < self.num_train_steps:
            log_fn(self.train_step())
        self.print('training complete')
