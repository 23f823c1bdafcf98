"""Drop-in for the reference's `utils` module: `from utils import *` (train.py:119) and
`from utils import init_predictor, DecodeCTCPred, Readf, ...` (predict.py:101-102) resolve to the
MI355X-native implementations.  Put this directory (crnn-ocr-lite_amd/) on sys.path in place of the
reference checkout."""
import numpy as np  # noqa: F401  (the reference's star-import also leaks np / os / re / pickle)
import os, re, gc, pickle, math, string  # noqa: F401,E401
from numpy.random import RandomState  # noqa: F401

from crnn_mi355x import optimizers  # noqa: F401  (utils.py:28 re-exports keras.optimizers)
from crnn_mi355x.surface import (CRNN, Model, init_predictor, load_custom_model, load_model_custom, save_model_json,  # noqa: F401
                                 model_from_json, ctc_lambda_func, BilinearInterpolation, STN, get_initial_weights)
from crnn_mi355x.decode import DecodeCTCPred, labels_to_text  # noqa: F401
from crnn_mi355x.lexicon import Lexicon, LexiconDecoder, lexicon_nearest  # noqa: F401  (beyond the reference: lexicon-constrained decoding on the device)
from crnn_mi355x.lm import CharLM, LMDecoder  # noqa: F401  (beyond the reference: beam search with a character language model, N-best)
from crnn_mi355x.align import CTCAligner, Alignment, CharSpan  # noqa: F401  (beyond the reference: character alignment on the device)
from crnn_mi355x.data import (Readf, open_img, read_img, norm, parse_mjsynth, get_lengths, get_lexicon, make_ohe)  # noqa: F401
from crnn_mi355x.ingest import DeviceIngest, DeviceReadf, plan_crop, box_slices  # noqa: F401  (beyond the reference: batches built on the device)
from crnn_mi355x.jpeg import JpegDecoder, jpeg_decode_host, jpeg_gray_host  # noqa: F401  (beyond the reference: baseline JPEG decoded on the device)
from crnn_mi355x.augment import AugmentPolicy, Augmenter, augment_host, neutral_items  # noqa: F401  (beyond the reference: training augmentation on the device)
from crnn_mi355x.synth import GlyphAtlas, SynthPolicy, SynthReadf, WordSynth, synth_host  # noqa: F401  (beyond the reference: training words rendered on the device)
from crnn_mi355x.detect import WordDetector, detect_words_host, reading_order  # noqa: F401  (beyond the reference: the word boxes, found on the device)
from crnn_mi355x.binarize import Binarizer, sauvola_host  # noqa: F401  (beyond the reference: adaptive binarisation in front of the detector)
from crnn_mi355x.deskew import Deskewer, deskew_host, estimate_skew_host, rotate_host  # noqa: F401  (beyond the reference: page deskew in front of the detector)
from crnn_mi355x.metrics import levenshtein, edit_distance, normalized_edit_distance  # noqa: F401
from crnn_mi355x.metrics import Score, device_edit_distances, check_label_metric  # noqa: F401  (beyond the reference: scored on the device)
from crnn_mi355x.metrics import edit_ops, confusion_matrix, device_edit_ops, Confusions  # noqa: F401  (edit scripts and character confusions)
from crnn_mi355x.callbacks import Callback, EarlyStoppingIter, ModelCheckpoint  # noqa: F401
