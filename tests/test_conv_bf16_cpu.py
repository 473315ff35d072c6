"""Host side of the opt-in bf16-operand 3x3 convs: the C ABI mirror, the conv_dtype model option, the Python scope."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instancediff_amd import _lib, ops  # noqa: E402
from instancediff_amd.models.drift_noise_model import parse_conv_dtype  # noqa: E402


def _header():
    with open(_lib.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_conv_desc_fields_match_the_header_struct():
    body = re.search(r"typedef struct \{(.*?)\} idiff_conv_desc;", _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        pieces = [p.strip() for p in decl.strip().split(",")] if decl.strip() else []
        if pieces:  # "type name" then ", name" ...
            names.append(re.findall(r"[A-Za-z_]\w*$", pieces[0])[0])
            names += [p.lstrip("*").strip() for p in pieces[1:]]
    assert [f[0] for f in _lib.ConvDesc._fields_] == names
    assert names[-2:] == ["wbf16", "operands"]


def test_algo_id_and_pack_symbols():
    hdr = _header()
    assert re.search(r"#define IDIFF_CONV_ALGO_BF16 6\b", hdr)
    assert ops.CONV_ALGO_BF16 == 6
    for s in ("idiff_pack_conv_weight_bf16", "idiff_conv_weight_bf16_bytes"):
        assert s in _lib.header_symbols() and s in _lib.SIGNATURES


def test_conv_dtype_option_is_parsed():
    assert parse_conv_dtype(None) == "f32"
    assert parse_conv_dtype("f32") == "f32"
    assert parse_conv_dtype("bf16") == "bf16"
    assert parse_conv_dtype("BF16") == "bf16"
    for bad in ("fp16", "bfloat16", "", 16, True):
        with pytest.raises(ValueError):
            parse_conv_dtype(bad)


def test_create_model_rejects_an_unknown_conv_dtype():
    from instancediff_amd import pipeline
    from instancediff_amd.models.drift_noise_model import create_CLIPDriftModel
    opt = pipeline.load_options()
    train_opt = dict(opt['train'])
    train_opt['dist'] = False
    model_opt = dict(opt['models'][train_opt['which_model']])
    model_opt['conv_dtype'] = "fp8"
    with pytest.raises(ValueError, match="conv_dtype"):
        create_CLIPDriftModel(train_opt, model_opt, phase="test", device="cpu")


def test_conv_operands_scope_is_thread_local_and_restored():
    import threading
    assert ops.current_conv_operands() == "f32"
    seen = []
    with ops.conv_operands("bf16"):
        assert ops.current_conv_operands() == "bf16"
        t = threading.Thread(target=lambda: seen.append(ops.current_conv_operands()))
        t.start()
        t.join()
        with ops.conv_operands("f32"):
            assert ops.current_conv_operands() == "f32"
        assert ops.current_conv_operands() == "bf16"
    assert ops.current_conv_operands() == "f32"
    assert seen == ["f32"]
    with pytest.raises(ValueError):
        with ops.conv_operands("fp16"):
            pass
