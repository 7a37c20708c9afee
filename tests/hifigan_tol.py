"""The parity tolerance of the HiFiGANGenerator tests and the file it is recorded in.

The tolerance is not fixed in advance: it is ONE TENTH OF THE SMALLEST PLANTED FAULT'S MOVEMENT -- every fault of hifigan_ref.FAULTS is
planted into the fp64 restatement of the two small configurations (2 x 17 frames, seed 0), its movement of the output measured as
max |delta| / RMS(reference), and a tenth of the smallest of them is what the device may differ from the restatement by.  A
kernel that made any of these mistakes would miss it ten times over.  tests/test_hifigan_cpu.py asserts the figures and that the
contract's own roundings stay inside half of it; tests/test_hifigan_gpu.py holds every whole-network case to it."""
import functools
import os

import hifigan_ref as H

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hifigan_parity.txt")
CONFIGS = ("SMALL", "SMALL2")


@functools.lru_cache(maxsize=None)
def parity_tolerance():
    """(tolerance, {(config, fault): movement}, {config: emulated-precision restatement vs fp64})"""
    moves, emu = {}, {}
    for name in CONFIGS:
        cfg = getattr(H, name)
        sd = H.random_state(cfg, 0)
        mel = H.mels(2, cfg["n_mels"], 17, 0)
        ref = H.generate(sd, cfg, mel)
        emu[name] = H.rel_err(H.generate(sd, cfg, mel, emulate=True), ref)
        for fault in H.FAULTS:
            if fault == "c2_dilated" and cfg["resblock"] != "1":
                continue  # ResBlock2 has no second convolution
            moves[(name, fault)] = H.rel_err(H.generate(sd, cfg, mel, fault=fault), ref)
    return min(moves.values()) / 10, moves, emu


def write_section(name, lines):
    """replace section `name` of profiles/hifigan_parity.txt (the CPU test's figures and the GPU test's live side by side); a tree
    that cannot be written to is left alone"""
    head, tail = f"== {name} ==", f"== end {name} =="
    try:
        text = open(PROFILE).read() if os.path.exists(PROFILE) else ""
        if head in text and tail in text:
            text = text[:text.index(head)] + text[text.index(tail) + len(tail) + 1:]
        text = text.rstrip("\n") + ("\n" if text.strip() else "") + "\n".join([head] + list(lines) + [tail]) + "\n"
        with open(PROFILE, "w") as fh:
            fh.write(text)
    except OSError:
        pass
