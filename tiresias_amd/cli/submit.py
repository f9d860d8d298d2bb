"""Submit a job to a running live cluster, or query / stop it.

The live runtime (``python -m tiresias_amd.cli.run_cluster --spool DIR``)
polls ``DIR`` every scheduling round (see ``executor/spool.py``).

Examples::

    python -m tiresias_amd.cli.submit --spool /tmp/tam --model resnet50 --gpus 2 --iterations 800
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model gnmt --duration 30 --grad-clip 5.0
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model transformer --iterations 800 --dropout 0.1 --attn-dropout 0.1
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model resnet50 --gpus 4 --iterations 800 --trust-ratio 0.001
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model resnet50 --batch 4 --iterations 800 --norm group
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model resnet50 --iterations 800 --cardinality 32
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model resnet50 --iterations 800 --se-ratio 16
    python -m tiresias_amd.cli.submit --spool /tmp/tam --model transformer --iterations 800 --pos rope
    python -m tiresias_amd.cli.submit --spool /tmp/tam --status
    python -m tiresias_amd.cli.submit --spool /tmp/tam --shutdown
"""
from __future__ import annotations

import argparse
import json
import sys

from ..executor.spool import Spool


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spool", required=True)
    ap.add_argument("--model")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--iterations", type=int)
    ap.add_argument("--duration", type=float, help="seconds of service (converted to iterations)")
    ap.add_argument("--job-id")
    ap.add_argument("--batch", type=int)
    ap.add_argument("--grad-clip", type=float,
                    help="clip the gradient's global L2 norm to this value; non-finite steps are skipped")
    ap.add_argument("--dropout", type=float,
                    help="training dropout probability at the model's dropout sites (0 <= p < 1)")
    ap.add_argument("--attn-dropout", type=float,
                    help="dropout probability on the attention probabilities, inside the attention kernels "
                         "(0 <= p < 1, quantised to 1/256: 0.1 drops 26/256); models without attention "
                         "dropout ignore it")
    ap.add_argument("--opt-dtype", choices=("fp32", "bf16", "factored"),
                    help="format of the optimizer state: bf16 keeps the moments in bf16 with stochastic "
                         "rounding (4 B per parameter less for Adam, 2 B for SGD, resident and spilled); "
                         "factored runs Adafactor on an Adam model (row and column means of the second "
                         "moment, no first moment: the state shrinks to O(rows + cols) per weight matrix; "
                         "not combined with --trust-ratio); default fp32")
    ap.add_argument("--trust-ratio", type=float, metavar="ETA",
                    help="layer-wise adaptive learning rates with trust coefficient ETA > 0: LARS for an SGD "
                         "model, LAMB for an Adam model; not combined with --opt-dtype bf16")
    ap.add_argument("--norm", choices=("batch", "group"),
                    help="normalisation of a ResNet job: group replaces every BatchNorm by a GroupNorm (32 "
                         "groups; per-sample statistics, so the result does not depend on the batch, the gang "
                         "width or packing); models without BatchNorm layers reject it; default batch")
    ap.add_argument("--cardinality", type=int, metavar="G",
                    help="ResNeXt variant of a ResNet job: every bottleneck's 3x3 conv runs in G groups (a multiple "
                         "of 4 in [4, 64]; resnet50 with 32 is ResNeXt-50 32x4d); other models reject it")
    ap.add_argument("--se-ratio", type=int, metavar="R",
                    help="Squeeze-and-Excitation variant of a ResNet job: every bottleneck gates its output per "
                         "(sample, channel) through two FCs C -> max(8, C / R) -> C (R in 4, 8, 16, 32; resnet50 "
                         "with 16 is SE-ResNet-50, with --cardinality 32 SE-ResNeXt-50 32x4d); other models "
                         "reject it")
    ap.add_argument("--pos", choices=("sinusoid", "rope"),
                    help="position encoding of a Transformer job: rope rotates Q and K inside the self-attention "
                         "kernels (rotary embeddings, pairs (j, j + 32), base 10000) in place of the additive "
                         "sinusoid table; other models reject it; default sinusoid")
    ap.add_argument("--status", action="store_true")
    ap.add_argument("--shutdown", action="store_true", help="stop serving once the cluster drains")
    a = ap.parse_args(argv)
    sp = Spool(a.spool)
    if a.status:
        print(json.dumps(sp.status(), indent=1))
        return 0
    if a.shutdown:
        sp.shutdown()
        print("shutdown requested")
        return 0
    if not a.model or (a.iterations is None and a.duration is None):
        ap.error("--model and one of --iterations / --duration are required")
    jid = sp.submit(a.model, a.gpus, iterations=a.iterations, duration=a.duration, job_id=a.job_id,
                    batch=a.batch, grad_clip=a.grad_clip, dropout=a.dropout,
                    attn_dropout=a.attn_dropout, opt_dtype=a.opt_dtype, trust_ratio=a.trust_ratio,
                    norm=a.norm, cardinality=a.cardinality, se_ratio=a.se_ratio, pos=a.pos)
    print(jid)
    return 0


if __name__ == "__main__":
    sys.exit(main())
