"""DurationPredictor training without a device: the fp64 restatement (tests/duration_train_ref.py) against a plain construction from
torch's own layers, the planted faults against the comparison and tolerances the GPU tests use, the host-side branch table of
DurationPredictor.forward in train() mode on CPU tensors, and the conditions the GPU tests' inputs rely on."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import aligner_ref
import duration_train_ref as R
from oracle import restate

import voicebox_pytorch_amd as vbx
from voicebox_pytorch_amd import _lib


def test_restatement_equals_plain_construction():
    """nn.Embedding / nn.Linear / nn.Conv1d / F.l1_loss around restate.transformer, the reference's lines :793-866 with the L1 on
    to_pred's output: the loss and every gradient to 1e-12"""
    case = R.given_case()
    sd = case["state"]
    E, D = sd["to_phoneme_emb.weight"].shape[1], 64
    emb, lin, pred = nn.Embedding(37, E), nn.Linear(D + E, D), nn.Linear(D, 1)
    conv = nn.Conv1d(D, D, 31, padding=15, groups=D)
    for mod, pre in ((emb, "to_phoneme_emb."), (lin, "to_embed."), (pred, "to_pred.0."), (conv, "conv_embed.dw_conv1d.0.")):
        mod.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
        mod.double()
    p = R.leaves(sd)
    cond, ids, cm = case["cond"].double(), case["ids"], case["cond_mask"]
    sam = ids != -1
    c = cond * (~cm)[..., None]
    x = lin(torch.cat((emb(ids.clamp(min=0)), c), dim=-1))
    xm = x.masked_fill(~sam[..., None], 0.0)
    x = F.gelu(conv(xm.transpose(1, 2))).transpose(1, 2).masked_fill(~sam[..., None], 0.0) + x
    x = restate.transformer(x, p, R.cfg_of(), mask=sam)
    d = pred(x)[..., 0]
    lm = cm & sam
    loss = F.l1_loss(d, case["target"], reduction="none").masked_fill(~lm, 0.0)
    loss = (loss.sum(-1) / lm.sum(-1).clamp(min=1e-5)).mean()
    loss.backward()
    ref = R.reference(case, emulate=False)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 * abs(float(ref["loss"]))
    plain = {"to_phoneme_emb.weight": emb.weight.grad, "to_embed.weight": lin.weight.grad, "to_embed.bias": lin.bias.grad,
             "to_pred.0.weight": pred.weight.grad, "to_pred.0.bias": pred.bias.grad,
             "conv_embed.dw_conv1d.0.weight": conv.weight.grad, "conv_embed.dw_conv1d.0.bias": conv.bias.grad}
    plain.update({k: v.grad for k, v in p.items() if k.startswith("transformer.") and torch.is_tensor(v) and v.grad is not None})
    assert len(plain) > 12
    for k, g in plain.items():
        assert R.rel_l2(g, ref["grads"][k]) <= 1e-12, (k, R.rel_l2(g, ref["grads"][k]))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_seen(fault):
    """every planted fault against the true restatement through compare(), with the GPU tests' tolerances.  "den_clamp_1" cannot
    move anything (a boolean mask has no denominator in (0, 1), and at 0 the numerator is 0): asserted as exactly that."""
    if fault in R.ALIGNER_FAULTS:
        case = R.aligner_case(flag=fault != "align_loss_always")
        tol = aligner_ref.tolerance()
    else:
        case, tol = R.given_case(), None
    good, bad = R.reference(case), R.reference(case, fault=fault)
    problems, figures = R.compare(bad, good, aligner_tol=tol)
    print(fault, problems[:4], max(figures.values()))
    assert R.compare(good, good, aligner_tol=tol)[0] == []
    if fault in R.INVISIBLE_FAULTS:
        assert problems == [] and float(bad["loss"]) == float(good["loss"])
        assert all(torch.equal(bad["grads"][k], g) for k, g in good["grads"].items() if g is not None)
    else:
        assert problems, fault


def test_input_conditions_hold_for_the_reference():
    """what the GPU tests rely on: planted targets at least 0.5 from a sign change on every case, the aligner case's predictions at
    least 0.4 from every integer, an empty loss-mask row, ragged padding with one full row, repeated ids, the fp64 training run"""
    for E, B, n, drop in R.GIVEN_CASES:
        c = R.given_case(E, B, n, drop)
        assert R.margin(c["d_ref"], c["target"]) >= 0.5 - 1e-9, (E, B, n, drop)
        lm = c["cond_mask"] & (c["ids"] != -1)
        assert bool(lm[0].any()) and bool((c["ids"][0] != -1).all())
        if B > 1:
            assert not bool(lm[-1].any()) and bool((c["ids"][1:] == -1).any())
        if n > 1:
            assert c["ids"].clamp(min=0).unique().numel() < c["ids"].numel()
    a = R.aligner_case()
    ref = R.reference(a)
    assert float((ref["d"] - 2.5).abs().max()) <= 0.1  # so |d - integer| >= 0.4
    assert float((ref["d"] - ref["target"]).abs().min()) >= 0.4
    assert a["aligner"]["klens"][1] < a["aligner"]["klens"][0] and a["aligner"]["qlens"][1] < a["aligner"]["qlens"][0]


def test_fp64_training_run_reaches_a_quarter():
    losses = R.train_run_ref(R.train_case())
    print("fp64 training run", R.TRAIN_LR, [round(l, 4) for l in losses])
    assert losses[-1] <= 0.25 * losses[0], (losses[0], losses[-1])


# ----------------------------------------------------------------------------- the host-side branch table
def _dp(attach=False):
    dp = vbx.DurationPredictor(num_phoneme_tokens=37, dim_phoneme_emb=24, dim=64, depth=2, dim_head=64, heads=2,
                               aligner_kwargs=dict(dim_in=16, attn_channels=8)).train()
    if attach:
        dp.attach_aligner()
    return dp


def _five(B=2, n=5, T=11):
    return dict(mel=torch.zeros(B, T, 16), phoneme_len=torch.full((B,), n), mel_len=torch.full((B,), T),
                phoneme_mask=torch.ones(B, 1, n, dtype=torch.int32), mel_mask=torch.ones(B, 1, T, dtype=torch.int32))


def test_valid_training_inputs_on_the_cpu_refuse_the_cpu():
    """given durations, and the aligner's five inputs: both reach the device check ("no CPU fallback")"""
    cond, ids = torch.zeros(2, 5, 64), torch.zeros(2, 5, dtype=torch.long)
    for dp, kw in ((_dp(), dict(target=torch.ones(2, 5))), (_dp(), dict(target=torch.ones(2, 5, dtype=torch.int64))),
                   (_dp(True), _five()), (_dp(True), dict(target=torch.ones(2, 5), **_five()))):
        with pytest.raises(_lib.VbxError, match="no CPU fallback"):
            dp(cond=cond, phoneme_ids=ids, **kw)


def test_training_branch_table():
    cond, ids = torch.zeros(2, 5, 64), torch.zeros(2, 5, dtype=torch.long)
    target = torch.ones(2, 5)
    with pytest.raises(NotImplementedError, match="target="):  # none of the five, no target
        _dp()(cond=cond, phoneme_ids=ids)
    with pytest.raises(NotImplementedError, match="target="):
        _dp(True)(cond=cond, phoneme_ids=ids)
    with pytest.raises(RuntimeError, match="attach_aligner"):  # the aligner branch without an aligner
        _dp()(cond=cond, phoneme_ids=ids, **_five())
    five = _five()
    for missing in five:  # some but not all: the reference's assertion
        part = {k: v for k, v in five.items() if k != missing}
        with pytest.raises(AssertionError, match="need to pass phoneme_len, mel_len, phoneme_mask, mel_mask, to train duration predictor module"):
            _dp(True)(cond=cond, phoneme_ids=ids, target=target, **part)
    with pytest.raises(AssertionError, match="need to pass"):
        _dp()(cond=cond, phoneme_ids=ids, mel=five["mel"])
    with pytest.raises(ValueError, match="length of phoneme_ids"):  # cond_mask & self_attn_mask cannot broadcast
        _dp()(cond=torch.zeros(2, 7, 64), phoneme_ids=ids, target=target)
    with pytest.raises(NotImplementedError, match="no gradient to cond"):
        _dp()(cond=cond.clone().requires_grad_(), phoneme_ids=ids, target=target)
    with pytest.raises(NotImplementedError, match="espeak"):  # texts / tokenizer: unchanged
        _dp()(cond=cond, texts=["hello"], target=target)
    with pytest.raises(NotImplementedError):
        vbx.DurationPredictor(num_phoneme_tokens=37, audio_enc_dec=object())
    dp = _dp()
    assert not dp.null_cond.requires_grad
    dp.eval()
    with pytest.raises(_lib.VbxError, match="no CPU fallback"):  # eval: as before
        dp(cond=cond, phoneme_ids=ids)
