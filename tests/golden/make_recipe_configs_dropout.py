"""Generate tests/golden/recipe_configs_dropout.json: the component config
lines the reference's own generator writes for the CTC recipe with
steps/ctc/train.sh --dropout-proportion 0.2.

Runs in the build container only, like make_recipe_configs.py beside it, whose
load_components / make_configs it uses (the same MakeConfigs call sequence);
the committed JSON is text data and is all that travels.

dropout_proportion is the float argparse gives make_configs.py for the shell's
"0.2" (type=float), which components.py:67-71 writes with str.format.
Configuration: BASELINE.json configs[1] (5 x BLSTM-512, max-seq-length 2000).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_recipe_configs import load_components, make_configs  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recipe_configs_dropout.json")


def main():
    nodes = load_components()
    cases = {
        "configs1": dict(feat_dim=40, num_targets=41, rnn_layers=5, cell_dim=512, rnn_mode=2, bidirectional=True,
                         max_seq_length=2000, dropout_proportion=float("0.2")),
    }
    out = {"generator": "egs/wsj/s5/steps/ctc/nnet2/components.py via tests/golden/make_recipe_configs_dropout.py",
           "args": cases,
           "configs": {k: make_configs(nodes, **v) for k, v in cases.items()}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, file=sys.stderr)


if __name__ == "__main__":
    main()
