"""The integer hash of the input side, stated once for the stages that use it (the augmentation's noise, the synthetic words' baseline
jitter; for the library: csrc/common.h crnn_mix32).  A leaf module."""
import numpy as np


def mix32(x):
    """The hash of include/crnn_mi355x.h on uint32 (arrays or scalars) -> uint64 values below 2^32."""
    m = np.uint64(0xffffffff)
    x = np.asarray(x, dtype=np.uint64) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x
