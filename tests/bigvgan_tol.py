"""The parity tolerance of the BigVGANGenerator tests and the file it is recorded in.

The tolerance is not fixed in advance: it is ONE TENTH OF THE SMALLEST PLANTED FAULT'S MOVEMENT -- every fault of NETWORK_FAULTS is
planted into the fp64 restatement of the two small configurations (2 x 17 frames, seed 0), its movement of the output measured as
max |delta| / RMS(reference), and a tenth of the smallest of them is what the device may differ from the restatement by.  The
condition (tests/test_bigvgan_cpu.py): the emulated-precision restatement's own distance from fp64 is at most half of it.

A fault that moves the output by less than 20 times that distance cannot be told from rounding by a whole-network test.  Two of
bigvgan_ref.FAULTS are of that kind -- they touch only the first and last few samples of each row, and the residual stream dilutes
them -- and are NOT in the whole-network list:
  up_zero_pad     zero instead of replicate padding in the up-sampler
  down_zero_pad   zero instead of replicate padding in the down-sampler
Both are covered by single-kernel tests instead, where they are far outside the per-element bound: on the host
tests/test_bigvgan_cpu.py::test_padding_faults_violate_the_activation_bound (each fault against the bound the device is held to), on
the device tests/test_bigvgan_gpu.py::test_activation, which holds vbx_bigvgan_act to that bound per element at rows shorter than
the filters' reach and at both ends of every row."""
import functools
import os

import bigvgan_ref as R

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bigvgan_parity.txt")
CONFIGS = ("SMALL", "SMALL2")
KERNEL_ONLY_FAULTS = ("up_zero_pad", "down_zero_pad")
NETWORK_FAULTS = tuple(f for f in R.FAULTS if f not in KERNEL_ONLY_FAULTS)


@functools.lru_cache(maxsize=None)
def parity_tolerance():
    """(tolerance, {(config, fault): movement} over ALL faults, {config: emulated-precision restatement vs fp64})"""
    moves, emu = {}, {}
    for name in CONFIGS:
        cfg = getattr(R, name)
        sd = R.random_state(cfg, 0)
        mel = R.mels(2, cfg["n_mels"], 17, 0)
        ref = R.generate(sd, cfg, mel)
        emu[name] = R.rel_err(R.generate(sd, cfg, mel, emulate=True), ref)
        for fault in R.FAULTS:
            if R.applies(fault, cfg):
                moves[(name, fault)] = R.rel_err(R.generate(sd, cfg, mel, fault=fault), ref)
    return min(v for (_, f), v in moves.items() if f in NETWORK_FAULTS) / 10, moves, emu


def write_section(name, lines):
    """replace section `name` of profiles/bigvgan_parity.txt (the CPU test's figures and the GPU test's live side by side); a tree
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
