"""What the decoders, the lexicon and the aligner share on the host side: the alphabet as {character: id}, label tables in the layout the
kernels read, and the way a softmax map gets onto the device.  Imports nothing from its users."""
import numpy as np

CHUNK = 4096                 # images per launch, and per upload of a host array
MAX_WORD_LEN = 31            # the library's max_len limit: 2 L + 1 <= 63 states, one per lane of a wavefront


def class_items(inverse_classes):
    """(id, character) pairs of {id: character} (what DecodeCTCPred holds) or of a list of characters"""
    return inverse_classes.items() if hasattr(inverse_classes, "items") else enumerate(inverse_classes)


class Alphabet:
    """.inverse_classes as given; .classes = {character: id}"""

    def __init__(self, inverse_classes):
        self.inverse_classes = inverse_classes
        self.classes = {str(ch): int(k) for k, ch in class_items(inverse_classes)}

    def encode(self, text):
        """-> list of label ids, or None for a text the kernels cannot take: a character outside the alphabet, or more than 31 of them."""
        if len(text) > MAX_WORD_LEN:
            return None
        ids = [self.classes.get(ch) for ch in text]
        return None if any(i is None for i in ids) else ids


def label_table(encoded):
    """[ids or None] -> (labels (n, width) int32 padded with -1, lengths (n,) int32); None gives length -1: an entry the kernels do not trust"""
    n = len(encoded)
    labels = np.full((n, max([len(e) for e in encoded if e is not None] + [1])), -1, dtype=np.int32)
    lengths = np.full(n, -1, dtype=np.int32)
    for i, e in enumerate(encoded):
        if e is not None:
            labels[i, :len(e)] = e; lengths[i] = len(e)
    return labels, lengths


def device_map(result, device=None):
    """ndarray or tensor -> contiguous float32 device tensor: a device tensor stays where it is, anything else goes to `device` (default: the current one)"""
    import torch
    y = result if torch.is_tensor(result) else torch.from_numpy(np.ascontiguousarray(result, dtype=np.float32))
    return (y if y.is_cuda else y.to(device or "cuda")).contiguous().float()


def decode_chunks(result, launch):
    """The decoders' loop over a map of any length: launch(chunk) -> a tuple of device tensors, for every CHUNK rows of `result` put on the device
    by device_map.  -> that tuple for the whole map (concatenated when there is more than one chunk), or None for an empty `result`."""
    import torch
    parts = [launch(device_map(result[lo:lo + CHUNK])) for lo in range(0, len(result), CHUNK)]
    if not parts:
        return None
    return parts[0] if len(parts) == 1 else tuple(torch.cat(p, 0) for p in zip(*parts))
