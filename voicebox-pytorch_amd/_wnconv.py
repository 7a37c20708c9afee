"""What the modules that load published weight-normed convolutions share (seanet.py, hifigan.py, bigvgan.py): the layer itself,
carried by its parameters, the one mapping of newer torch's parameter names onto weight_g / weight_v, and the reader of a local
config.json."""
import json
import os

from torch import nn

_PARAM = "parametrizations.weight.original"


def weight_norm_key(key):
    """newer torch's parametrizations.weight.original0 / original1 -> weight_g / weight_v; any other key as it is"""
    for n, name in enumerate(("weight_g", "weight_v")):
        if key.endswith(_PARAM + str(n)):
            return key[:-len(_PARAM) - 1] + name
    return key


def read_config(config):
    """a config.json as a dict: None and a dict as they are, anything else as a LOCAL path"""
    if config is None or isinstance(config, dict):
        return config
    with open(os.fspath(config)) as fh:
        return json.load(fh)


def _norm(w):
    """|w| over all but dim 0, [n, 1, 1]: per output channel of a convolution [Co, Ci, k], per INPUT channel of a transposed one
    [Ci, Co, k] -- torch's weight norm at its default dim=0"""
    return w.flatten(1).norm(dim=1).reshape(-1, 1, 1)


class WNConv(nn.Module):
    """nn.Conv1d or nn.ConvTranspose1d by its parameters, initialised as torch initialises that layer: weight_g [n, 1, 1] / weight_v /
    bias under weight norm; weight / bias without (weight_norm=False, or after plain_(True): a checkpoint saved after
    remove_weight_norm).  `bias` may be set to None."""

    def __init__(self, cin, cout, k, dilation=1, stride=1, transposed=False, weight_norm=True):
        super().__init__()
        self.cin, self.cout, self.k, self.dilation, self.stride, self.transposed = cin, cout, k, dilation, stride, transposed
        ref = nn.ConvTranspose1d(cin, cout, k, stride=stride) if transposed else nn.Conv1d(cin, cout, k)
        self._set_weight(ref.weight.detach(), weight_norm)
        self.bias = nn.Parameter(ref.bias.detach().clone())

    def _set_weight(self, w, weight_norm):
        if weight_norm:
            self.weight_g = nn.Parameter(_norm(w))
            self.weight_v = nn.Parameter(w.clone())
        else:
            self.weight = nn.Parameter(w.clone())

    def plain_(self, plain):
        """switch between the weight_g / weight_v and the plain `weight` parametrisation, keeping the folded weight"""
        if plain == hasattr(self, "weight"):
            return
        w = self.folded()
        if plain:
            del self.weight_g, self.weight_v
        else:
            del self.weight
        self._set_weight(w, not plain)

    def folded(self):
        """fp32 w = g * v / |v|; a plain weight as it is"""
        if hasattr(self, "weight"):
            return self.weight.detach().float()
        v = self.weight_v.detach().float()
        return self.weight_g.detach().float() * v / _norm(v)
