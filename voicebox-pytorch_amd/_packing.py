"""What the codec modules with device-side operand copies share (vocos.py, seanet.py, codec.py): the key that says when a copy
is out of date, the cache around it, and the reader of a local checkpoint."""
import torch


def read_checkpoint(path):
    """the state dict of a LOCAL torch.save file: the dict itself or its 'state_dict' entry"""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd


def tensors_key(tensors):
    """(storage address, version counter) per tensor: it moves with an in-place update, load_state_dict and .to().  An inference
    tensor has no counter and cannot be written in place.  A write through `.data` changes neither."""
    return tuple((t.data_ptr(), 0 if t.is_inference() else t._version) for t in tensors)


class PackedWeights:
    """Mixin of an nn.Module that keeps operands packed from its weights: _cached(build) returns build()'s result and calls it again
    only when _weights_key() moved (by default over every parameter) or after mark_weights_dirty(), which a caller owes after a
    write through `p.data`."""

    _packed, _packed_key = None, None

    def _weights_key(self):
        return tensors_key(self.parameters())

    def mark_weights_dirty(self):
        self._packed_key = None

    def _cached(self, build):
        key = self._weights_key()
        if key != self._packed_key:
            self._packed, self._packed_key = build(), key
        return self._packed
