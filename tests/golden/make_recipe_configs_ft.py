"""Generate tests/golden/recipe_configs_ft.json: the component config lines the
reference's own generator writes for the CTC recipe with
steps/ctc/train.sh --model-type FT and / or --add-lda true.

Runs in the build container only, like make_recipe_configs.py beside it, whose
load_components it uses; the committed JSON is text data and is all that
travels.

The call sequence restates MakeConfigs (make_configs.py:237-358) for
rnn_first, splice_indexes "0 0 0 ...":
  init.config = AddInputLayer
                [+ AddLdaLayer(lda_dim or the spliced dim, <config_dir>/../lda.mat)]
                [+ AddAffRelNormLayer(hidden_dim) + AddClipGradientLayer]      (FT)
                + AddRnnLayer(first) + AddAffineLayer(num_targets)
  layer{i}.config, softmax.config as in make_recipe_configs.py
with train.sh's values: affine_type "native", active_type "relu", hidden_dim
1024, self_repair_scale 0.00001 (argparse float), batch_normalize False,
clipping_threshold 30.0, norm_based_clipping True; config_dir is the recipe's
<dir>/configs.
Configuration: BASELINE.json configs[1] (5 x BLSTM-512, max-seq-length 2000).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_recipe_configs import load_components  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recipe_configs_ft.json")
CONFIG_DIR = "exp/ctc_ft/configs"


def make_configs(nodes, feat_dim, num_targets, rnn_layers, cell_dim, rnn_mode, bidirectional, max_seq_length,
                 model_type="google", add_lda=False, lda_dim=0, hidden_dim=1024, affine_type="native",
                 self_repair_scale=0.00001, batch_normalize=False, cudnn_layers=1, param_stddev=0.02,
                 bias_stddev=0.2, clipping_threshold=30.0, norm_based_clipping=True, dropout_proportion=0.0):
    files = {}
    init = {"components": []}
    prev = nodes.AddInputLayer(init, feat_dim, [0], 0)
    if add_lda:
        if lda_dim <= 0:
            lda_dim = prev["dimension"]
        prev = nodes.AddLdaLayer(init, lda_dim, CONFIG_DIR + "/../lda.mat")
    if model_type == "FT":
        prev = nodes.AddAffRelNormLayer(init, prev, hidden_dim, affine_type=affine_type,
                                        self_repair_scale=self_repair_scale, batch_normalize=batch_normalize)
        prev = nodes.AddClipGradientLayer(init, prev, clipping_threshold=clipping_threshold,
                                          norm_based_clipping=norm_based_clipping,
                                          self_repair_scale_clipgradient=None)
    first = nodes.AddRnnLayer(init, prev, cell_dim, num_layers=cudnn_layers, max_seq_length=max_seq_length,
                              bidirectional=bidirectional, rnn_mode=rnn_mode,
                              clipping_threshold=clipping_threshold, dropout_proportion=dropout_proportion,
                              norm_based_clipping=norm_based_clipping, self_repair_scale_clipgradient=None)
    nodes.AddAffineLayer(init, first, num_targets)
    files["init.config"] = init["components"]
    out = first
    for i in range(rnn_layers - 1):
        lines = {"components": []}
        out = nodes.AddRnnLayer(lines, out, cell_dim, num_layers=cudnn_layers, max_seq_length=max_seq_length,
                                bidirectional=bidirectional, rnn_mode=rnn_mode, param_stddev=param_stddev,
                                bias_stddev=bias_stddev, clipping_threshold=clipping_threshold,
                                dropout_proportion=dropout_proportion, norm_based_clipping=norm_based_clipping,
                                self_repair_scale_clipgradient=None)
        files[f"layer{i + 1}.config"] = lines["components"]
    files["softmax.config"] = [f"SoftmaxComponent dim={num_targets}"]
    return files


def main():
    nodes = load_components()
    base = dict(feat_dim=40, num_targets=41, rnn_layers=5, cell_dim=512, rnn_mode=2, bidirectional=True,
                max_seq_length=2000)
    cases = {
        "ft": dict(base, model_type="FT", hidden_dim=1024),
        "add_lda": dict(base, add_lda=True, lda_dim=0),
        "ft_add_lda": dict(base, model_type="FT", hidden_dim=1024, add_lda=True, lda_dim=30),
    }
    out = {"generator": "egs/wsj/s5/steps/ctc/nnet2/components.py via tests/golden/make_recipe_configs_ft.py",
           "args": cases,
           "config_dir": CONFIG_DIR,
           "configs": {k: make_configs(nodes, **v) for k, v in cases.items()}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, file=sys.stderr)


if __name__ == "__main__":
    main()
