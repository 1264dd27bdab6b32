#!/usr/bin/env python3
"""Generate tests/golden/caffe_neuron_fields.json: the field NAMES that the reference's schema declares for the parameter
messages of the neuron layers (tests/neuron_cases.py gives every one of them a disposition).

Run in the authoring container only (needs the reference tree), like make_layer_fields.py, whose reading of the schema this
uses:

    python tests/golden/make_neuron_fields.py [OUTDIR]

It reads caffe/src/caffe/proto/caffe.proto at generation time and writes names only: no types, no defaults, no comments.
No test reads the reference tree."""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_layer_fields as M  # noqa: E402

MESSAGES = ["PReLUParameter", "ELUParameter", "PowerParameter", "ExpParameter", "LogParameter", "ThresholdParameter",
            "SigmoidParameter", "TanHParameter"]


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
    with open(M.PROTO) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    fields = {name: M.top_level_fields(M.message_body(text, name)) for name in MESSAGES}
    with open(os.path.join(outdir, "caffe_neuron_fields.json"), "w") as f:
        json.dump(fields, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
