"""CPU tests (no GPU) of alphabets beyond 64 classes: the library plans a workspace for up to 128 classes (two classes per lane of a
wavefront in the softmax / CTC / beam kernels) and refuses 129, the parameter layout and the Keras artefacts carry a 97-class dense2, and
the label -> text mapping reaches the ids of the upper half."""
import ctypes
import json

import numpy as np
import pytest

import utils as U
from crnn_mi355x import native
from crnn_mi355x.surface import param_layout, _cfg_struct


def _ws_bytes(num_classes, precision):
    lib = native.lib()
    lib.crnn_workspace_bytes.restype = ctypes.c_size_t
    cfg = _cfg_struct(8, (100, 32, 1), num_classes, 23, 128, 256, False)
    cfg.mfma_bf16 = precision
    return int(lib.crnn_workspace_bytes(ctypes.byref(cfg)))


@pytest.mark.parametrize("precision", [0, 1, 2])          # fp32 (parity), bf16 products, bf16 products and storage
def test_workspace_is_planned_for_2_to_128_classes_and_refused_outside(precision):
    for C in (65, 97, 128):
        assert _ws_bytes(C, precision) > 0, C
    assert _ws_bytes(38, precision) > 0 and _ws_bytes(64, precision) > 0
    assert _ws_bytes(129, precision) == 0 and _ws_bytes(1, precision) == 0


def test_parameter_layout_of_a_97_class_model():
    lay = param_layout(_cfg_struct(8, (100, 32, 1), 97, 23, 128, 256, False))
    assert lay["dense2_w"][2] == (512, 97) and lay["dense2_b"][2] == (97,)
    assert list(lay)[-2:] == ["dense2_w", "dense2_b"]


def test_97_class_model_json_and_hdf5_weights_round_trip(tmp_path):
    m = U.CRNN(num_classes=97, shape=(100, 32, 1)).get_model()
    rs = np.random.RandomState(3)
    ws = [rs.normal(size=w.shape).astype(np.float32) for w in m.get_weights()]
    m.set_weights(ws)
    assert ws[-2].shape == (512, 97) and ws[-1].shape == (97,)
    (tmp_path / "m97").mkdir()
    U.save_model_json(m, str(tmp_path), "m97")
    text = open(tmp_path / "m97" / "model.json").read()
    dense2 = [l for l in json.loads(text)["config"]["layers"] if l["class_name"] == "Dense"][-1]
    assert dense2["config"]["units"] == 97
    m2 = U.model_from_json(text)
    assert m2.config == m.config and m2.config["num_classes"] == 97
    assert json.loads(m2.to_json()) == json.loads(text)
    path = str(tmp_path / "m97" / "final_weights.h5")
    m.save_weights(path)
    m2.load_weights(path)
    got = m2.get_weights()
    assert len(got) == len(ws) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, ws))
    m3 = U.load_custom_model(str(tmp_path / "m97"))
    assert m3.config["num_classes"] == 97 and all(np.array_equal(a, b) for a, b in zip(m3.get_weights(), ws))


def test_labels_to_text_reaches_the_upper_half_of_a_96_character_alphabet():
    chars = [chr(33 + i) for i in range(96)]                 # '!' .. '\x80': 96 distinct one-character strings
    inv = dict(enumerate(chars))
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv)
    ids = list(range(64, 96))
    assert dec.labels_to_text(ids) == "".join(chars[64:96]) and len(dec.labels_to_text(ids)) == 32
    assert dec.labels_to_text([96]) == "" and dec.labels_to_text([-1]) == "" and dec.labels_to_text([96, -1, 96]) == ""
    assert dec.labels_to_text(np.array([95, 96, 0, -1, 64], dtype=np.int32)) == chars[95] + chars[0] + chars[64]
    assert U.labels_to_text([64, 96, 95, -1], inv) == chars[64] + chars[95]
