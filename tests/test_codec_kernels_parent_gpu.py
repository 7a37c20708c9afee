"""The codec kernels (csrc/mel.hip, csrc/griffinlim.hip, csrc/seanet.hip) give the bits they gave before their shared parts moved
into csrc/fft_lds.hpp and sn_tile_product: tests/golden/codec_kernels_parent.json holds one SHA-256 of the raw output bytes per case,
recorded on the parent commit by tests/golden/make_codec_kernels_parent.py, whose cases() rebuilds the inputs here (closed form,
no RNG).  Several outputs pass through libm (expm1f, log10f, hypotf), so a hash only means something under the toolchain that
produced it: where torch.version.hip or the `HIP version` line of hipcc --version differ from the recorded ones the whole test
skips and names both; under the recorded toolchain every case is compared and none is skipped."""
import importlib.util
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_codec_kernels_parent", os.path.join(HERE, "golden", "make_codec_kernels_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_codec_kernels_give_the_parents_bits():
    maker = _maker()
    with open(os.path.join(HERE, "golden", "codec_kernels_parent.json")) as fh:
        rec = json.load(fh)
    recorded, running = (rec["torch_version_hip"], rec["hipcc_version"]), maker.toolchain()
    if running != recorded:
        pytest.skip(f"hashes recorded under {recorded}, running under {running}")
    want, compared, wrong = rec["sha256"], 0, []
    for name, fn in maker.cases():
        assert name in want, f"case {name!r} is not in the recorded file"
        got = fn()
        torch.cuda.synchronize()
        compared += 1
        if maker.sha(got) != want[name]:
            wrong.append(name)
    assert compared == len(want) == 59
    assert not wrong, f"{len(wrong)} of {compared} outputs differ from the parent's: {wrong}"
