"""LoRA adapters on the device: fine-tune a pretrained VoiceBox by training W0 + (alpha / r) . B . A on the four big matrices of a layer.

The adapters act on the fp32 MASTER weights: while they are attached, the adapted matrix's slot of the flat parameter buffer holds
W_eff = W0 + s . B . A, so every forward, backward and sampler kernel (which all read packed copies of the master weights) serves the
adapted model unchanged and at no cost per forward.  What is new lives in csrc/lora.hip: the merge (vbx_lora_apply) and the kernel that
turns the weight gradient dW the backward already writes into dA and dB (vbx_lora_grad).  dp.TrainStep drives both.

    vb.add_lora(rank=16, alpha=16.)           # freezes the base, registers lora_A / lora_B on the adapted nn.Linear modules
    step = TrainStep(wrapper); step.step(x1)  # only the adapters (and whatever else requires grad) move
    vb.lora_state_dict() / vb.load_lora_state_dict(sd)
    vb.merge_lora()                           # drop the adapters, keep W_eff
    vb.detach_lora()                          # drop the adapters, restore W0 bit for bit
"""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib
from ._lib import F, I

TARGETS = {"to_qkv": "QKVW", "to_out": "OUTW", "ff_in": "FF1W", "ff_out": "FF2W"}  # target name -> slot of engine.L_NAMES
MAX_RANK = 64
W0_BUFFER = "_lora_w0"  # non-persistent buffer on the VoiceBox: follows .to(), stays out of state_dict()


class VbxLoraDesc(C.Structure):  # vbx_lora_desc of include/vbx.h
    _fields_ = [("w_off", C.c_long), ("w0_off", C.c_long), ("a_off", C.c_long), ("b_off", C.c_long), ("N", I), ("K", I), ("r", I),
                ("scale", F), ("blk0", C.c_long), ("tile0", C.c_long), ("red0", C.c_long), ("pa_off", C.c_long), ("pb_off", C.c_long)]


def _align64(n):
    return (n + 63) // 64 * 64


class LoraTable:
    """A descriptor table checked and filled by vbx_lora_plan (host), plus its device copy once `to(device)` was called."""

    def __init__(self, rows, flat_floats, w0_floats, lflat_floats):
        """rows: [(w_off, w0_off, a_off, b_off, N, K, r, scale), ...]"""
        self.n = len(rows)
        self.host = (VbxLoraDesc * self.n)()
        for d, (w_off, w0_off, a_off, b_off, N, K, r, scale) in zip(self.host, rows):
            d.w_off, d.w0_off, d.a_off, d.b_off, d.N, d.K, d.r, d.scale = w_off, w0_off, a_off, b_off, N, K, r, scale
        ab, gt, rb, sf = C.c_long(0), C.c_long(0), C.c_long(0), C.c_long(0)
        mr, mk = C.c_int(0), C.c_int(0)
        _lib.call("vbx_lora_plan", self.host, self.n, int(flat_floats), int(w0_floats), int(lflat_floats), C.byref(ab), C.byref(gt),
                  C.byref(rb), C.byref(sf), C.byref(mr), C.byref(mk))
        self.apply_blocks, self.grad_tiles, self.reduce_blocks, self.scratch_floats = ab.value, gt.value, rb.value, sf.value
        self.max_rank, self.max_k = mr.value, mk.value
        self.dev = None

    def to(self, device):
        if self.dev is None or self.dev.device != torch.device(device):
            self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)
        return self

    def apply(self, flat, w0, lflat):
        _lib.call("vbx_lora_apply", flat, w0, lflat, self.to(flat.device).dev, self.n, self.apply_blocks, self.max_k, _lib.current_stream())

    def grad(self, gflat, lflat, glflat, scratch):
        assert scratch.numel() >= self.scratch_floats and glflat.numel() >= lflat.numel()
        _lib.call("vbx_lora_grad", gflat, lflat, glflat, self.to(gflat.device).dev, self.n, self.grad_tiles, self.reduce_blocks,
                  self.max_rank, scratch, _lib.current_stream())


class LoraState:
    """What VoiceBox._lora holds while adapters are attached."""

    def __init__(self, vb, rank, alpha, entries, saved_flags):
        self.vb, self.rank, self.alpha, self.scale = vb, int(rank), float(alpha), float(alpha) / int(rank)
        self.entries = entries          # dicts: layer, target, slot, module, key (state-dict key of the weight), N, K, a_off, b_off, w0_off
        self.saved_flags = saved_flags  # [(parameter, requires_grad before add_lora)]
        self.lnumel = _align64(entries[-1]["b_off"] + entries[-1]["N"] * rank)
        self.w0numel = entries[-1]["w0_off"] + _align64(entries[-1]["N"] * entries[-1]["K"])
        self.lflat = None
        self.needs_apply = False
        self.applied_key = None
        self._table = None
        self.hooks = []

    # -- storage
    def params(self):
        for e in self.entries:
            yield e["module"].lora_A
            yield e["module"].lora_B

    def key(self):
        return sum(p._version for p in self.params())

    @property
    def w0(self):
        return getattr(self.vb, W0_BUFFER)

    def w0_view(self, e):
        return self.w0[e["w0_off"]:e["w0_off"] + e["N"] * e["K"]].view(e["N"], e["K"])

    def ensure(self, device):
        """The adapter parameters as views into ONE flat fp32 buffer on `device` (re-flattened after .to(), like FlatParams)."""
        ok = self.lflat is not None and self.lflat.device == device
        if ok:
            base = self.lflat.data_ptr()
            for e in self.entries:
                a, b = e["module"].lora_A, e["module"].lora_B
                if a.data_ptr() != base + 4 * e["a_off"] or b.data_ptr() != base + 4 * e["b_off"] or a.dtype != torch.float32:
                    ok = False
                    break
        if ok:
            return self.lflat
        with torch.inference_mode(False), torch.no_grad():
            lflat = torch.zeros(self.lnumel, dtype=torch.float32, device=device)
            for e in self.entries:
                for p, off in ((e["module"].lora_A, e["a_off"]), (e["module"].lora_B, e["b_off"])):
                    view = lflat[off:off + p.numel()].view(p.shape)
                    view.copy_(p.data.to(device=device, dtype=torch.float32))
                    p.data = view
        self.lflat = lflat
        self._table = None
        return lflat

    def table(self):
        fp = self.vb.flat_params()
        if self._table is None:
            rows = [(fp.offsets[e["slot"]], e["w0_off"], e["a_off"], e["b_off"], e["N"], e["K"], self.rank, self.scale) for e in self.entries]
            self._table = LoraTable(rows, fp.numel, self.w0numel, self.lnumel)
        return self._table

    # -- W_eff = W0 + s . B . A into the master slots
    def apply(self):
        """Re-applies the adapters (vbx_lora_apply) and bumps the weights epoch so that every engine and captured sampler repacks.
        On a CPU model nothing can be launched: the merge is left pending and runs when the model next builds an engine."""
        fp = self.vb.flat_params()
        dev = fp.flat.device
        lflat = self.ensure(dev)
        if dev.type != "cuda":
            self.needs_apply = True
            return
        if self.w0.device != dev:
            setattr(self.vb, W0_BUFFER, self.w0.to(dev))
        self.table().apply(fp.flat, self.w0, lflat)
        self.needs_apply, self.applied_key = False, self.key()
        fp.bump()

    def sync(self):
        """Host check (no device sync): re-apply when a loader left the merge pending or an adapter was written through the parameter."""
        if self.needs_apply or self.key() != self.applied_key:
            self.apply()

    def require_merged(self, what):
        if self.needs_apply or self.key() != self.applied_key:
            self.apply()
        if self.needs_apply:
            raise _lib.VbxError(f"{what}: the adapters were changed on a CPU model and the merge W0 + s.B.A runs only on an MI355X "
                                "(vbx_lora_apply; there is no CPU fallback) -- move the model to the GPU first")

    # -- state dicts
    def _sd_hook(self, module, sd, prefix, local_metadata):
        for e in self.entries:  # W0 under the reference's keys; the adapter keys are ordinary parameters of the adapted nn.Linear
            k = prefix + e["key"]
            if k in sd:
                sd[k] = self.w0_view(e).detach().clone()

    def _load_hook(self, module, incompatible):
        # the slots now hold what the dict had under the weight keys: the (new) base.  A plain dict has no adapter keys: not an error.
        missing = incompatible.missing_keys
        missing[:] = [k for k in missing if not (k.endswith(".lora_A") or k.endswith(".lora_B"))]
        with torch.no_grad():
            for e in self.entries:
                self.w0_view(e).copy_(e["module"].weight.detach().to(self.w0.device))
        self.needs_apply = True
        self.apply()


def refuse_autograd(vb):
    """With adapters attached the eager autograd path would hand out dW for the frozen W_eff and nothing for A and B."""
    if getattr(vb, "_lora", None) is not None:
        raise NotImplementedError("LoRA adapters are attached: they train through dp.TrainStep (and VoiceBoxTrainer) only -- the eager "
                                  "autograd path (wrapper(x1).backward()) has no adapter gradients.  Build a TrainStep over the wrapper, "
                                  "or call merge_lora() / detach_lora() first")


def add_lora(vb, rank=16, alpha=16., targets=("to_qkv", "to_out", "ff_in", "ff_out"), layers=None, train_base=False):
    from .engine import precise_enabled

    # every refusal before anything is touched or launched
    if getattr(vb, "_lora", None) is not None:
        raise ValueError("add_lora: adapters are already attached -- merge_lora() or detach_lora() first")
    if precise_enabled():
        raise NotImplementedError("add_lora: precise mode does not serve LoRA adapters -- leave precise mode")
    targets = tuple(targets)
    if "to_qkva" in targets:
        raise NotImplementedError("add_lora: GateLoop's to_qkva is not an adapter target (to_qkv, to_out, ff_in, ff_out are)")
    unknown = [t for t in targets if t not in TARGETS]
    if unknown or not targets:
        raise ValueError(f"add_lora: unknown targets {unknown}; the targets are {', '.join(TARGETS)}")
    if not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
        raise NotImplementedError(f"add_lora: rank must be an integer in 1 .. {MAX_RANK} (got {rank!r})")
    L = vb._cfg["L"]
    layers = list(range(L)) if layers is None else sorted(set(int(l) for l in layers))
    if not layers or layers[0] < 0 or layers[-1] >= L:
        raise ValueError(f"add_lora: layers must be indices in 0 .. {L - 1}")
    fp = vb.flat_params()
    dev = fp.flat.device
    entries, loff, woff = [], 0, 0
    for l in layers:
        _, _, _, attn, _, ff = vb.transformer.layers[l]
        mods = {"to_qkv": (attn.to_qkv, f"transformer.layers.{l}.3.to_qkv.weight"), "to_out": (attn.to_out, f"transformer.layers.{l}.3.to_out.weight"),
                "ff_in": (ff[0], f"transformer.layers.{l}.5.0.weight"), "ff_out": (ff[3], f"transformer.layers.{l}.5.3.weight")}
        for t in TARGETS:
            if t not in targets:
                continue
            mod, key = mods[t]
            N, K = mod.weight.shape
            e = dict(layer=l, target=t, slot=f"L{l}.{TARGETS[t]}", module=mod, key=key, N=int(N), K=int(K), a_off=loff,
                     b_off=loff + _align64(rank * K), w0_off=woff)
            loff = e["b_off"] + _align64(N * rank)
            woff += _align64(N * K)
            entries.append(e)
    saved = [(p, p.requires_grad) for p in vb.parameters()]
    st = LoraState(vb, rank, alpha, entries, saved)
    with torch.no_grad():
        w0 = torch.zeros(st.w0numel, dtype=torch.float32, device=dev)
        lflat = torch.zeros(st.lnumel, dtype=torch.float32, device=dev)
        for e in entries:
            w0[e["w0_off"]:e["w0_off"] + e["N"] * e["K"]].copy_(e["module"].weight.detach().reshape(-1))
            a = lflat[e["a_off"]:e["a_off"] + rank * e["K"]].view(rank, e["K"])
            nn.init.kaiming_uniform_(a, a=math.sqrt(5))  # as nn.Linear initialises a weight; B = 0: W_eff = W0 bit for bit, no launch
            e["module"].register_parameter("lora_A", nn.Parameter(a))
            e["module"].register_parameter("lora_B", nn.Parameter(lflat[e["b_off"]:e["b_off"] + e["N"] * rank].view(e["N"], rank)))
    st.lflat = lflat
    vb.register_buffer(W0_BUFFER, w0, persistent=False)
    if not train_base:
        for p, _ in saved:
            p.requires_grad_(False)
    for e in entries:  # the adapted matrices themselves are always frozen: their slot holds W_eff, a function of (W0, A, B)
        e["module"].weight.requires_grad_(False)
    st.applied_key = st.key()
    reg = getattr(vb, "register_state_dict_post_hook", None) or vb._register_state_dict_hook
    # (plain functions: torch marks a public state-dict hook with an attribute, which a bound method does not take)
    st.hooks = [reg(lambda module, sd, prefix, meta: st._sd_hook(module, sd, prefix, meta) and None),
                vb.register_load_state_dict_post_hook(lambda module, incompatible: st._load_hook(module, incompatible))]
    vb._lora = st
    return vb


def _remove(vb):
    st = vb._lora
    for h in st.hooks:
        h.remove()
    for e in st.entries:
        del e["module"]._parameters["lora_A"]
        del e["module"]._parameters["lora_B"]
    del vb._buffers[W0_BUFFER]
    vb._non_persistent_buffers_set.discard(W0_BUFFER)
    for p, flag in st.saved_flags:  # the requires_grad flags of before add_lora
        p.requires_grad_(flag)
    vb._lora = None


def _attached(vb, what):
    st = getattr(vb, "_lora", None)
    if st is None:
        raise ValueError(f"{what}: no adapters are attached (add_lora first)")
    return st


def merge_lora(vb):
    """Drops the adapters and keeps W_eff: a plain model with a plain state dict (the requires_grad flags of before add_lora return)."""
    st = _attached(vb, "merge_lora")
    st.require_merged("merge_lora")
    _remove(vb)
    return vb


def detach_lora(vb):
    """Drops the adapters and restores W0 bit for bit."""
    st = _attached(vb, "detach_lora")
    fp = vb.flat_params()
    with torch.no_grad():
        for e in st.entries:
            e["module"].weight.data.copy_(st.w0_view(e).to(fp.flat.device))
    fp.bump()
    _remove(vb)
    return vb


def lora_state_dict(vb):
    """Adapters only: the adapted weight's state-dict key with .weight -> .lora_A / .lora_B."""
    st = _attached(vb, "lora_state_dict")
    out = {}
    for e in st.entries:
        stem = e["key"][:-len("weight")]
        out[stem + "lora_A"] = e["module"].lora_A.detach().clone()
        out[stem + "lora_B"] = e["module"].lora_B.detach().clone()
    return out


def load_lora_state_dict(vb, sd):
    st = _attached(vb, "load_lora_state_dict")
    want = {}
    for e in st.entries:
        stem = e["key"][:-len("weight")]
        want[stem + "lora_A"], want[stem + "lora_B"] = e["module"].lora_A, e["module"].lora_B
    missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or extra:
        raise ValueError(f"load_lora_state_dict: missing keys {missing}, unexpected keys {extra}")
    for k, p in want.items():
        if tuple(sd[k].shape) != tuple(p.shape):
            raise ValueError(f"load_lora_state_dict: {k} has shape {tuple(sd[k].shape)}, the adapter has {tuple(p.shape)}")
    with torch.no_grad():
        for k, p in want.items():
            p.copy_(sd[k])
    st.needs_apply = True
    st.apply()
    return vb
