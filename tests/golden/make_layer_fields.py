#!/usr/bin/env python3
"""Generate tests/golden/caffe_layer_fields.json: the field NAMES that the reference's schema declares for the messages the
graph reader has to account for (tests/graph_field_cases.py gives every one of them a disposition).

Run in the authoring container only (needs /root/reference), like make_golden.py:

    python tests/golden/make_layer_fields.py [OUTDIR]

It reads caffe/src/caffe/proto/caffe.proto at generation time and writes names only: no types, no defaults, no comments.
No test reads the reference tree."""
import json
import os
import re
import sys

PROTO = "/root/reference/caffe/src/caffe/proto/caffe.proto"
MESSAGES = ["NetParameter", "LayerParameter", "ConvolutionParameter", "PoolingParameter", "ReLUParameter", "EltwiseParameter",
            "CropParameter", "BatchNormParameter", "ScaleParameter", "NormalizeParameter", "ConcatParameter",
            "SoftmaxParameter", "ReshapeParameter", "PythonParameter", "InputParameter"]
_FIELD = re.compile(r"^\s*(?:optional|repeated|required)\s+[\w.]+\s+(\w+)\s*=\s*\d+", re.M)


def message_body(text, name):
    m = re.search(r"^message\s+%s\s*\{" % re.escape(name), text, re.M)
    if not m:
        raise SystemExit("message %s not found in %s" % (name, PROTO))
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def top_level_fields(body):
    """Field names of the message itself: nested enum / message bodies are cut out first."""
    out, depth, keep = [], 0, []
    for ch in body:
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif depth == 0:
            keep.append(ch)
    for m in _FIELD.finditer("".join(keep)):
        out.append(m.group(1))
    return out


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
    with open(PROTO) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    fields = {name: top_level_fields(message_body(text, name)) for name in MESSAGES}
    with open(os.path.join(outdir, "caffe_layer_fields.json"), "w") as f:
        json.dump(fields, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
