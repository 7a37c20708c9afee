"""HiFiGANMelCodec.encode / mel_spectrogram: the native kernel (csrc/mel.hip, vbx_melspec, one launch) beside the same arithmetic as a
user would write it without it -- HiFi-GAN's mel_spectrogram from F.pad(mode="reflect") + torch.stft(center=False) + sqrt + matmul +
log on the same device in fp32.  HiFi-GAN's V1 configuration (n_fft 1024, hop 256, 80 mels, 22.05 kHz, fmax 8000).  One MI355X.

    python tools/hifigan_mel_times.py [OUT.json]                   (default: profiles/hifigan_mel_times.json)

One process: per shape the arms run alternating, after warm-up, device events around windows of back-to-back calls (the host side of
a call included); the minimum of the five windows is the figure, every window and their spread are recorded.  Nothing is asserted
about which arm wins."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 262144, 50), (1, 77056, 50)]  # B, samples, calls per window
REPS, WARM = 5, 10
V1 = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)


def main():
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F

    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.codec import melspec_pad, slaney_mel_filterbank

    dev = "cuda"
    codec = vbx.HiFiGANMelCodec(**V1)
    n_fft, hop, win = V1["n_fft"], V1["hop_size"], V1["win_size"]
    pad = melspec_pad(n_fft, hop)
    fb = slaney_mel_filterbank(n_fft, V1["num_mels"], V1["sampling_rate"], V1["fmin"], V1["fmax"]).float().to(dev)
    hann = torch.hann_window(win, device=dev)

    def torch_arm(y):
        y = F.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
        spec = torch.view_as_real(torch.stft(y, n_fft, hop_length=hop, win_length=win, window=hann, center=False, normalized=False,
                                             onesided=True, return_complex=True))
        return torch.log(torch.clamp(torch.matmul(fb, torch.sqrt(spec.pow(2).sum(-1) + 1e-9)), min=1e-5))

    arms = {"native_encode_frames_major": codec.encode, "native_mel_spectrogram_channel_first": lambda y: vbx.mel_spectrogram(y, **V1),
            "torch_pad_stft_matmul_log_fp32": torch_arm}

    def window(fn, y, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn(y)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    res = {"device": torch.cuda.get_device_name(0), "config": V1, "protocol": f"arms alternating in one process, {REPS} windows of back-to-back "
           f"calls after {WARM} warm-up calls, device events, host side included; ms per call", "shapes": {}}
    for B, T, calls in SHAPES:
        torch.manual_seed(0)
        y = torch.randn(B, T, device=dev) * 0.3
        for fn in arms.values():
            for _ in range(WARM):
                fn(y)
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(REPS):
            for k, fn in arms.items():
                times[k].append(window(fn, y, calls))
        row = {k: dict(min_ms=min(v), max_ms=max(v), median_ms=sorted(v)[len(v) // 2], spread=(max(v) - min(v)) / min(v), windows_ms=v,
                       calls_per_window=calls) for k, v in times.items()}
        row["frames"] = int(codec.encode(y).shape[1])
        row["torch_over_native_channel_first"] = row["torch_pad_stft_matmul_log_fp32"]["min_ms"] / \
            row["native_mel_spectrogram_channel_first"]["min_ms"]
        row["max_abs_difference_between_arms"] = float((vbx.mel_spectrogram(y, **V1) - torch_arm(y)).abs().max())
        res["shapes"][f"{B}x{T}"] = row
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hifigan_mel_times.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
