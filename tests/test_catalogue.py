"""The filter catalogue against its recording on the parent commit.

tests/data/catalogue_parent.json is the output of tools/record_catalogue.py on
the commit before the parser became a token table and the stencil list a single
X-macro: what every token of the recorder's fixed list parsed to or was refused
with, what it compiled to, the stencil weights and `ops.FILTERS`.  The current
build must reproduce all of it; only the list of syntaxes behind an "unknown
filter" message may differ, in order and separators.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import record_catalogue  # noqa: E402  (tools/)


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(HERE, "data", "catalogue_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    return json.loads(json.dumps(record_catalogue.record()))


def test_recorder_covers_the_recorded_tokens(parent):
    assert record_catalogue.tokens() == list(parent["tokens"])
    for tok in ("median7", "open", "erode3:1", "gradient", "tophat3:2", "unsharp:0", "unsharp:1:9",
                "threshold:adaptive:7", "threshold:otsu:1", "blend:2", "lincomb:9:0", "above:300", "bilateral7",
                "bilateral3:0", "autocontrast:50", "colormatrix:1;0;0;0;1;0;0;0", "equalize@skip", "hold@constant",
                "gray,,invert", "foo"):
        assert "ok" not in parent["tokens"][tok], tok
    assert any(t.startswith("conv:4:") for t in parent["tokens"])
    assert sum("ok" in r for r in parent["tokens"].values()) > 300


def test_every_recorded_value_is_reproduced(parent, current):
    for tok, want in parent["tokens"].items():
        assert current["tokens"][tok] == want, tok
    assert current["stencil_weights"] == parent["stencil_weights"]
    assert current["stencils"] == parent["stencils"] and current["aliases"] == parent["aliases"]


def test_filters_is_the_catalogue(C, parent):
    import mpi_cuda_imagemanipulation_amd as m

    pairs = [list(kv) for kv in m.ops.FILTERS.items()]
    assert pairs == [list(kv) for kv in C.filter_catalogue()] == parent["filters"]


def test_stencil_names_and_aliases_round_trip(C, parent):
    names = C.stencil_names()
    assert names == parent["stencils"]
    for name in names:  # the canonical text is the name, with its default where the filter has a parameter
        assert C.parse_chain(name).split(":")[0] == name
    for alias, name in parent["aliases"].items():
        assert C.parse_chain(alias) == C.parse_chain(name)
        assert C.stencil_weights(alias) == C.stencil_weights(name)
    for spelling in [*names, *parent["aliases"]]:
        text = C.parse_chain(spelling)
        assert C.parse_chain(text) == text


def test_unknown_filter_message_names_the_catalogue(C, parent):
    rows = [syntax for syntax, _ in C.filter_catalogue()]
    for tok, want in parent["tokens"].items():
        if "unknown" not in want:
            continue
        with pytest.raises(RuntimeError) as e:
            C.parse_chain(tok)
        msg = record_catalogue.message(e.value)
        assert msg.startswith(want["unknown"] + " ("), tok
        for syntax in rows:
            assert syntax in msg, (tok, syntax)
    assert sum("unknown" in r for r in parent["tokens"].values()) > 30
