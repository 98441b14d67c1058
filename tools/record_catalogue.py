#!/usr/bin/env python3
"""Record what the filter catalogue of the built package accepts, rejects and means.

    python tools/record_catalogue.py [--out tests/data/catalogue_parent.json]

The token list is fixed and lives in this file.  For every token the record
holds `_C.parse_chain`'s canonical text or its error message (without the
leading `file:line: `, which moves with the code; of an "unknown filter"
message the part up to the name, the list of syntaxes after it once), for
accepted tokens `_C.describe_chain` on 1 and 3 input channels (text or error)
and, where the token has one, `_C.color_matrix` / `_C.bilateral_table`; for
every stencil name and alias `_C.stencil_weights`; and `ops.FILTERS` as a list
of pairs.

tests/data/catalogue_parent.json is the output of this script on the commit
before the catalogue became table-driven; tests/test_catalogue.py holds every
later build to it.  Re-record only when a filter is added or changed on purpose.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STENCILS = ["emboss3", "emboss5", "gaussian3", "gaussian5", "gaussian7", "box3", "box5", "sharpen", "laplace",
            "sobel", "sobel_l2", "median3", "median5", "erode3", "erode5", "dilate3", "dilate5", "bilateral3",
            "bilateral5"]
ALIASES = {"emboss": "emboss3", "gaussian": "gaussian5", "gauss5": "gaussian5", "laplacian": "laplace",
           "edge": "sobel", "magnitude": "sobel_l2", "median": "median3", "erode": "erode3", "dilate": "dilate3",
           "bilateral": "bilateral5"}
BORDERS = ["reflect101", "replicate", "constant", "skip"]

CONV3 = "conv:3:0;1;0;1;-4;1;0;1;0"
SEPCONV3 = "sepconv:3:0.25;0.5;0.25:1;2;1"
CM = "colormatrix:1;0;0;0;0.5;0.5;0.25;0.25;0.5"

# every FILTERS key as concrete tokens, every alias, every optional argument with and without it
ACCEPTED = [
    "gray", "gray:ref", "gray:bt601", "gray:cv", "grayscale", "grey:ref",
    "contrast", "contrast:3.5", "contrast:3:cv", "contrast:2:round", "contrast:2:ref", "contrast:2:trunc",
    "contrast:1.25", "contrast:-1",
    "invert", "negate", "brightness:40", "brightness:-40", "bright:10", "brightness:2.9",
    "threshold", "threshold:77", "threshold:128", "threshold:0", "expand", "gray2rgb",
    CM, CM + ":10;-20;0.5", "colormatrix:-7.99;0;0;0;7.99;0;0;0;0.0001:2048;-2048;0",
    "sepia", "saturation:1.5", "saturate:0.5", "saturation:0", "saturation:1", "saturation:-2", "swaprb", "bgr",
    "ycbcr", "ycbcr:inv",
    "equalize", "autocontrast", "autocontrast:0", "autocontrast:1", "autocontrast:2.5", "autocontrast:49.99",
    "autocontrast:0.004", "threshold:otsu",
    *STENCILS, *ALIASES,
    "open3", "open5", "close3", "close5",
    "bilateral3:10", "bilateral5:25", "bilateral:3.5", "bilateral5:4096", "bilateral3:10000", "bilateral3:0.1",
    "bilateral5:12.75",
    "blur", "blur:5", "blur:31", "blur:9:2.0", "blur:5:lsb", "blur:5:exact", "blur:7:1.5:lsb", "gblur:5", "blur:67",
    "blur:3", "blur:lsb",
    CONV3, CONV3 + ":lsb", CONV3 + ":exact", "conv:1:2",
    SEPCONV3, SEPCONV3 + ":lsb", SEPCONV3 + ":exact",
    "hold", "save", "swap", "add", "sub", "rsub", "absdiff", "min", "max",
    "lincomb:0.5:0.5", "lincomb:1:-1:10", "lincomb:-7.99:7.99:-2048", "lincomb:1:1:0", "blend:0.25", "blend:0",
    "blend:1", "blend:0.3333",
    "above", "above:0", "above:5", "above:-255", "above:255",
    "gradient3", "gradient5", "tophat3", "tophat5", "blackhat3", "blackhat5",
    "unsharp", "unsharp:1", "unsharp:1.5", "unsharp:2:3", "unsharp:0.5:7", "unsharp:6.99:5", "unsharp:0.0002",
    "threshold:adaptive:3", "threshold:adaptive:5", "threshold:adaptive:5:7", "threshold:adaptive:3:-10",
    "threshold:adaptive:3:255",
    # trailing arguments that today's parser ignores
    "gaussian5:1", "sobel:x", "invert:5", "expand:1", "gray:ref:extra", "contrast:1:cv:extra", "brightness:1:2",
    "threshold:5:6", "emboss:3", "negate:x:y",
    # presets, and chains that hold them
    "ref-gpu", "ref-cpu", "ref-gpu,expand", "ref-cpu,expand", "gray,ref-cpu", "invert,ref-gpu,invert",
    # chains: the canonical text joins, sugar expands in place
    "gray:ref,contrast:3.5,emboss3", "hold,gaussian5,sub", "hold,open3,sub,threshold:otsu", "gradient3,unsharp:1.5",
    "median,erode,dilate,bilateral", "gray,tophat5@replicate,expand", "hold,swap,hold,add",
    # whitespace
    " gaussian5 ", "gray , invert", "\tgray:ref ,\ncontrast:3.5, emboss3 ", "conv:3: 0; 1 ;0;1;-4;1;0;1;0",
    "conv:3:0;1;0;1;-4;1;0;1;0: lsb ", "blur:5: lsb", "blur: 5", "unsharp: 1.5 : 3", "lincomb: 0.5 :0.5",
    "blend: 0.5", "above: 3", "threshold: adaptive :3: 2", "threshold: otsu", "threshold: 5", "ycbcr: inv",
    "saturation: 1.5", "autocontrast: 2", "bilateral3: 10", "sepconv:3: 1;2;1 : 1; 0;-1", CM.replace(";", " ; "),
    "brightness: 7", "contrast: 2",
]

# @border on one token of each kind (and the spellings of the border modes)
BORDER_HEADS = ["gaussian5", "emboss", "sobel_l2", "median3", "dilate", "bilateral3:10", "bilateral", "blur:5",
                "blur:5:lsb", CONV3, SEPCONV3, "open3", "close5", "gradient3", "tophat5", "blackhat3", "unsharp",
                "unsharp:2:3", "threshold:adaptive:3", "threshold:adaptive:5:4", "invert", "gray:ref", "contrast:2:cv",
                "brightness:5", "threshold:9", "expand", "sepia", CM, "saturation:2", "swaprb", "ycbcr:inv",
                # refused with a border: statistic, slot and combine ops
                "equalize", "autocontrast", "autocontrast:2", "threshold:otsu", "hold", "save", "swap", "add", "sub",
                "rsub", "absdiff", "min", "max", "lincomb:1:1", "blend:0.5", "above", "above:3",
                "ref-gpu", "ref-cpu"]
BORDER_SPELLINGS = ["reflect", "default", "clamp", "zero", "legacy"]

REJECTED = [
    # sized families
    "median7", "median33", "medianx", "open", "close", "open7", "opening", "erode3:1", "erodes", "dilate9",
    "dilate5:x", "open3:1", "close5:2", "median:1",
    "gradient", "gradient7", "gradientx", "tophat", "tophat3:2", "blackhat", "blackhat9", "blackhat5:1",
    "bilateral7", "bilateralx", "bilateral3:0", "bilateral3:-1", "bilateral5:10001", "bilateral3:abc",
    "bilateral3:1:2", "bilateral7:5",
    # sugar with arguments
    "unsharp:0", "unsharp:7", "unsharp:-1", "unsharp:1:9", "unsharp:1:4", "unsharp:1:5:2", "unsharp:x",
    "unsharp:0.0001",
    "threshold:adaptive", "threshold:adaptive:7", "threshold:adaptive:x", "threshold:adaptive:3:1.5",
    "threshold:adaptive:3:300", "threshold:adaptive:3:1:2", "threshold:adaptive:3:x",
    "threshold:otsu:1", "threshold:x", "threshold:",
    # combine and slot ops
    "blend", "blend:2", "blend:-0.1", "blend:0.5:1", "blend:x", "lincomb", "lincomb:1", "lincomb:9:0",
    "lincomb:0:-9", "lincomb:1:1:3000", "lincomb:1:1:1:1", "lincomb:a:b", "above:300", "above:-256", "above:1.5",
    "above:1:2", "above:x", "add:1", "min:2", "absdiff:x", "swap:1", "save:1", "hold:0",
    # pointwise and colour
    "autocontrast:50", "autocontrast:-1", "autocontrast:1:2", "autocontrast:49.999", "autocontrast:x", "equalize:1",
    "brightness", "brightness:x", "bright", "gray:foo", "contrast:1:foo", "contrast:abc", "contrast:",
    "colormatrix", "colormatrix:1;0;0;0;1;0;0;0", "colormatrix:1;0;0;0;1;0;0;0;1;0", CM + ":1;2", CM + ":1;2;3;4",
    CM + ":1;2;3:4", "colormatrix:9;0;0;0;1;0;0;0;1", "colormatrix:1;0;0;0;1;0;0;0;x", CM + ":3000;0;0",
    "sepia:1", "bgr:1", "swaprb:x", "saturation", "saturate", "saturation:100", "saturation:-100", "saturation:x",
    "saturation:1:2", "ycbcr:fwd", "ycbcr:inv:1",
    # float convolutions
    "blur:4", "blur:1", "blur:69", "blur:5:1:2", "blur:5:1:2:lsb", "blur:x", "blur:5:x",
    "conv", "conv:3", "conv:4:" + ";".join(["1"] * 16), "conv:3:1;2", "conv:3:" + ";".join(["1"] * 10),
    CONV3 + ":fast", CONV3 + ":lsb:1", "conv:69:1", "conv:x:1", "conv:3:0;1;0;1;x;1;0;1;0", "conv:-1:1",
    "sepconv", "sepconv:3:1;1;1", "sepconv:3:1;1:1;1;1", "sepconv:3:1;1;1:1;1;1;1", "sepconv:4:1;1;1;1:1;1;1;1",
    "sepconv:3:1;1;1:1;1;1:fast", "sepconv:69:1:1", "sepconv:3:1;x;1:1;1;1",
    # borders
    "equalize@skip", " equalize@skip ", "autocontrast:1@replicate", "threshold:otsu@constant", "hold@constant",
    "save@skip", "swap@replicate", "add@skip", "lincomb:1:1@constant", "blend:0.5@skip", "above@reflect101",
    "gaussian5@foo", "gaussian5@", "gaussian5@skip@skip", "gaussian5 @replicate", "gaussian5@ replicate", "@skip",
    "foo@bar", "foo@skip", "unsharp@skip:1", "median7@foo", "ref-gpu@skip", "ref-cpu@replicate",
    "threshold:5 @skip", "open@skip", "bilateral3:0@skip",
    # presets with arguments, empty tokens, unknown names
    "ref-gpu:1", "ref-cpu:x", "ref", "ref-", "", " ", ",", "gray,,invert", "gray,", ",gray", "gray, ,invert",
    "foo", "Gaussian5", "gaussian9", "box7", "gauss3", "sobel_l1", "emboss7", "holdx", "adds", "minimum", "swaps",
    "sepiax", "grayx", "blurs", "convx", "thresholds", "lincombx", ":", ":1", "gaussian5;sobel",
]


def tokens() -> list[str]:
    out = list(ACCEPTED)
    for head in BORDER_HEADS:
        out += [f"{head}@{b}" for b in BORDERS]
    out += [f"gaussian5@{b}" for b in BORDER_SPELLINGS] + [f"open3@{b}" for b in BORDER_SPELLINGS]
    out += REJECTED
    seen, uniq = set(), []
    for t in out:
        if t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


_PREFIX = re.compile(r"^[^\s:']+\.(?:cpp|h|hip):\d+: ")


def message(e: BaseException) -> str:
    """The error text without the `file:line: ` that STRIPE_CHECK puts in front."""
    return _PREFIX.sub("", str(e))


def attempt(fn, *args):
    try:
        return {"ok": fn(*args)}
    except RuntimeError as e:
        return {"error": message(e)}


def record() -> dict:
    sys.path.insert(0, ROOT)
    import mpi_cuda_imagemanipulation_amd as m

    C = m._C
    toks, tails = {}, set()
    for t in tokens():
        r = attempt(C.parse_chain, t)
        if r.get("error", "").startswith("unknown filter '"):
            # the list of syntaxes that follows the name is the same every time: kept once
            head, sep, tail = r["error"].partition("' (")
            r = {"unknown": head + "'"}
            tails.add(sep[1:] + tail)
        if "ok" in r:
            r["describe"] = {str(cin): attempt(C.describe_chain, t, cin) for cin in (1, 3)}
            for key, fn in (("color_matrix", C.color_matrix), ("bilateral_table", C.bilateral_table)):
                v = attempt(fn, t)
                if "ok" in v:
                    r[key] = v["ok"]
        toks[t] = r
    return {
        "filters": [list(kv) for kv in m.ops.FILTERS.items()],
        "stencils": STENCILS,
        "aliases": ALIASES,
        "stencil_weights": {n: C.stencil_weights(n) for n in [*STENCILS, *ALIASES]},
        "unknown_filter_tail": sorted(tails),
        "tokens": toks,
    }


def dump(rec: dict) -> str:
    """JSON with one catalogue row, stencil or token per line (readable diffs)."""
    def rows(d):
        if isinstance(d, dict):
            return "{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in d.items()) + "\n }"
        return "[\n" + ",\n".join("  " + json.dumps(v) for v in d) + "\n ]"

    body = ",\n".join(f" {json.dumps(k)}: {rows(v) if k in ('filters', 'stencil_weights', 'tokens') else json.dumps(v)}"
                      for k, v in rec.items())
    return "{\n" + body + "\n}\n"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "data", "catalogue_parent.json"))
    a = ap.parse_args()
    rec = record()
    assert json.loads(dump(rec)) == json.loads(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(dump(rec))
    n_ok = sum("ok" in r for r in rec["tokens"].values())
    print(f"{a.out}: {len(rec['tokens'])} tokens ({n_ok} accepted), {len(rec['filters'])} catalogue rows")


if __name__ == "__main__":
    main()
