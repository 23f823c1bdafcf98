"""DecodeCTCPred (utils.py:331-357): softmax maps -> text.  The reference loops over samples in Python and
builds one TF beam-search op + session.run per image (1.01 s/image, README.md:75); here the whole batch is
decoded by one launch of the HIP wavefront beam kernel (csrc/beam.hip), with TF-1.8 semantics including
merge_repeated=True ('cellist' decodes to 'celist', as in the reference's own screenshots)."""
import numpy as np

from .labels import decode_chunks


def labels_to_text(labels, inverse_classes=None):
    """utils.py:314-321: blank (== len(inverse_classes)) or -1 -> ''."""
    blank = len(inverse_classes)
    return "".join("" if (c == blank or c == -1) else str(inverse_classes[int(c)]) for c in labels)


class DecodeCTCPred:

    def __init__(self, top_paths=1, beam_width=5, inverse_classes=None, merge_repeated=True, greedy=False):
        self.top_paths = top_paths
        self.beam_width = beam_width
        self.inverse_classes = inverse_classes
        self.merge_repeated = merge_repeated     # TF-1.8 default, not overridden by Keras 2.2.2
        self.greedy = greedy                     # K.ctc_decode(greedy=True) variant (BASELINE config 2)

    def labels_to_text(self, labels):
        return labels_to_text(labels, self.inverse_classes)

    def decode_labels(self, result, device=False):
        """(N,T,C) softmax -> (N,T) int labels padded with -1 (device kernels; one launch per chunk).  A device tensor is decoded where it
        is; an ndarray is uploaded chunk by chunk.  device=True: -> (labels (N,T), lengths (N,)) int32 DEVICE tensors, nothing copied back
        (what metrics.device_edit_distances reads)."""
        import torch
        from . import engine
        if self.beam_width < self.top_paths:
            self.beam_width = self.top_paths
        run = engine.greedy_decode if self.greedy else (lambda chunk: engine.beam_decode(chunk, self.beam_width, self.merge_repeated)[:2])
        done = decode_chunks(result, run if device else (lambda chunk: (run(chunk)[0].cpu(),)))      # host labels come back chunk by chunk
        if done is None:
            if device:
                return torch.zeros((0, 0), dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
            return np.zeros((0, 0), np.int32)
        return done if device else done[0].numpy()

    def decode(self, result):
        return [self.labels_to_text(row) for row in self.decode_labels(result)]
