"""The per-job training knobs: ONE table, read by everything that carries them.

A knob is a part of a job's training recipe that the job asks for
(``submit --grad-clip``, a spool request's ``"grad_clip"`` key) and that
travels request -> ``ReplayJob`` field -> start action -> ``Trainer``
keyword under one name. Which knobs exist, what values are legal, which
models they apply to, how they travel and whether they fix a trainer's
buffers is decided by the rows of ``KNOBS`` and by ``check_together``; the
submit CLI, the spool, the controller, the worker, the trainer and the fake
backend loop over the table.

A new knob is one row here, a ``ModelSpec`` field, a ``ReplayJob`` field and
a ``Trainer`` keyword (plus a ``Trainer.set_<name>`` unless it is structural).

This module imports neither torch nor ``tiresias_amd.models`` when it is
loaded (the submit CLI and the spool import it); the checks look ``MODELS``
up when they run.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Any, Callable, Dict, Optional, Union


@dataclass(frozen=True)
class Knob:
    # the request key, the start action's key, the Trainer keyword and the
    # ReplayJob field
    name: str
    # model-independent check of a value that is not None, fit for untrusted
    # JSON (bools, wrong types, NaN and inf are refused): returns the value
    # as the trainer takes it, ValueError otherwise
    value: Callable[[Any], Any]
    # argparse keywords of the submit CLI's --<name> option
    cli: Dict[str, Any]
    # (model, value) -> None, ValueError when a job of that model cannot run
    # with the value; None: every model takes every legal value
    applies: Optional[Callable[[str, Any], None]] = None
    # the ModelSpec field a Trainer falls back on
    spec_field: str = ""
    # what None means
    default: Any = None
    # a STRUCTURAL knob fixes the trainer's "model" (its layers, or its
    # forward and with it the captured graph) or its optimizer-state
    # "buffers": it is set at construction and is part of the worker's
    # warm-pool key, and there is no per-job setter, because a pooled trainer
    # built with another value cannot serve the job. None: a per-job knob,
    # set on new and on pooled trainers alike through Trainer.set_<name>
    fixes: Optional[str] = None
    # structural knobs: the warm-pool key's token for a value that is not the
    # default (the default adds nothing, so a job that asks for nothing keeps
    # the key it always had), and how a pooled trainer of that value is named
    token: str = ""
    label: str = ""
    # the request / start-action key is written only when the job asks (a job
    # that does not: the file and the action as they always were); otherwise
    # it is always written, null when off
    sparse: bool = False
    # why a value other than the default is not supported on a multi-GPU gang
    # under ddp_shard (by value where the reasons differ); None: it is
    sharded: Union[None, str, Dict[Any, str]] = None

    def __post_init__(self):
        object.__setattr__(self, "spec_field", self.spec_field or self.name)
        object.__setattr__(self, "label", self.label or self.token)


# ------------------------------------------------------------------ value checks
def _finite_positive(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0 or v == float("inf"):
        raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    return float(v)


def _probability(name: str, steps: int, v) -> float:
    """A dropout probability the kernels can draw: quantised to 1/``steps``,
    and the quantised value is still below 1."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < 1 or round(v * steps) >= steps:
        raise ValueError(f"{name} must be a number p with 0 <= p < 1 (quantised to 1/{steps}), got {v!r}")
    return float(v)


def _one_of(name: str, choices: tuple, says: str, v) -> str:
    if not isinstance(v, str) or v not in choices:
        raise ValueError(f"{name} must be {says}, got {v!r}")
    return v


def _cardinality(v) -> int:
    from ..models.cnn import check_cardinality_value

    check_cardinality_value(v)
    return v


def _se_ratio(v) -> int:
    from ..models.cnn import check_se_ratio_value

    check_se_ratio_value(v)
    return v


# ------------------------------------------------------------------ applicability checks
def _offered(name: str, attr: str, lacks: str, model: str, v) -> None:
    """The model's builder says what it offers: a tuple of values (``norms``,
    ``positions``) or True for every legal value (``cardinalities``,
    ``se_ratios``); a builder without the attribute offers nothing."""
    from ..models import MODELS

    offers = getattr(MODELS[model].builder, attr, ())
    if not (offers is True or v in (offers or ())):
        raise ValueError(f"{name}={v!r}: {model!r} {lacks}")


def _factored_needs_adam(model: str, v) -> None:
    from ..models import MODELS

    if v == "factored" and MODELS[model].opt != "adam":
        raise ValueError(f"opt_dtype 'factored' (Adafactor) needs an adam model, {model!r} is not one")


_OPT_DTYPES = ("fp32", "bf16", "factored", "q8")
_NORMS = ("batch", "group")
_POSITIONS = ("sinusoid", "rope")

KNOBS: Dict[str, Knob] = {k.name: k for k in (
    # global-norm gradient clip (README "gradient clipping")
    Knob("grad_clip", partial(_finite_positive, "grad_clip"), spec_field="clip",
         sharded="a sharded gang's global norm needs the replicated tails counted once",
         cli=dict(type=float,
                  help="clip the gradient's global L2 norm to this value; non-finite steps are skipped")),
    # training dropout at the model's dropout sites; a model without them ignores it
    Knob("dropout", partial(_probability, "dropout", 65536),
         cli=dict(type=float, help="training dropout probability at the model's dropout sites (0 <= p < 1)")),
    Knob("attn_dropout", partial(_probability, "attn_dropout", 256),
         cli=dict(type=float,
                  help="dropout probability on the attention probabilities, inside the attention kernels "
                       "(0 <= p < 1, quantised to 1/256: 0.1 drops 26/256); models without attention "
                       "dropout ignore it")),
    # format of the optimizer state (README "bf16 optimizer state", "Factored
    # optimizer state", "8-bit optimizer state"): the state buffers of one
    # format cannot serve a job of another
    Knob("opt_dtype", partial(_one_of, "opt_dtype", _OPT_DTYPES,
                              "'fp32' or 'bf16', 'q8' for 8-bit block-scaled state, or 'factored' for an adam model"),
         applies=_factored_needs_adam, default="fp32", fixes="buffers", token="{}", label="{}-state",
         sharded={"bf16": "the sharded gang's slice launches and state all-gather are fp32-state only",
                  "factored": "a sharded member holds only slices of the rows its row and column means run over",
                  "q8": "a sharded member holds slices that cut the 256-element quantisation blocks"},
         cli=dict(choices=_OPT_DTYPES,
                  help="format of the optimizer state: bf16 keeps the moments in bf16 with stochastic "
                       "rounding (4 B per parameter less for Adam, 2 B for SGD, resident and spilled); "
                       "factored runs Adafactor on an Adam model (row and column means of the second "
                       "moment, no first moment: the state shrinks to O(rows + cols) per weight matrix; "
                       "not combined with --trust-ratio); q8 keeps Adam's or SGD's own update and stores "
                       "every moment as one code byte per element plus one fp32 scale per 256 elements, with "
                       "stochastic rounding (about 6 B per parameter less for Adam, 3 B for SGD; not combined "
                       "with --trust-ratio); default fp32")),
    # layer-wise trust coefficient: LARS (sgd models) / LAMB (adam models)
    Knob("trust_ratio", partial(_finite_positive, "trust_ratio"),
         sharded="a sharded member holds only slices of the segments its norms run over",
         cli=dict(type=float, metavar="ETA",
                  help="layer-wise adaptive learning rates with trust coefficient ETA > 0: LARS for an SGD "
                       "model, LAMB for an Adam model; not combined with --opt-dtype bf16 or q8")),
    # normalisation of a CNN job (README "GroupNorm"): "group" builds the
    # model with GroupNorm in place of every BatchNorm: other layers, no
    # running statistics
    Knob("norm", partial(_one_of, "norm", _NORMS, "'batch' or 'group'"),
         applies=partial(_offered, "norm", "norms", "has no BatchNorm layers (the knob is for the ResNet models)"),
         default="batch", fixes="model", token="norm={}", sparse=True,
         cli=dict(choices=_NORMS,
                  help="normalisation of a ResNet job: group replaces every BatchNorm by a GroupNorm (32 "
                       "groups; per-sample statistics, so the result does not depend on the batch, the gang "
                       "width or packing); models without BatchNorm layers reject it; default batch")),
    # ResNeXt cardinality of a ResNet job (README "ResNeXt"): G builds every
    # bottleneck with a G-group 3x3 conv on the grouped conv kernels
    Knob("cardinality", _cardinality,
         applies=partial(_offered, "cardinality", "cardinalities",
                         "has no bottleneck 3x3 conv to group (the knob is for the ResNet models)"),
         fixes="model", token="cardinality={}", sparse=True,
         cli=dict(type=int, metavar="G",
                  help="ResNeXt variant of a ResNet job: every bottleneck's 3x3 conv runs in G groups (a multiple "
                       "of 4 in [4, 64]; resnet50 with 32 is ResNeXt-50 32x4d); other models reject it")),
    # Squeeze-and-Excitation ratio of a ResNet job (README "SE blocks"): r
    # adds an SE block (four parameters, the se.hip kernels) to every bottleneck
    Knob("se_ratio", _se_ratio,
         applies=partial(_offered, "se_ratio", "se_ratios",
                         "has no bottleneck to put an SE block on (the knob is for the ResNet models)"),
         fixes="model", token="se_ratio={}", sparse=True,
         cli=dict(type=int, metavar="R",
                  help="Squeeze-and-Excitation variant of a ResNet job: every bottleneck gates its output per "
                       "(sample, channel) through two FCs C -> max(8, C / R) -> C (R in 4, 8, 16, 32; resnet50 "
                       "with 16 is SE-ResNet-50, with --cardinality 32 SE-ResNeXt-50 32x4d); other models "
                       "reject it")),
    # position encoding of a Transformer job (README "rotary position
    # embeddings"): "rope" rotates Q and K inside the self-attention kernels
    # in place of the additive table. No parameter moves, but the model's
    # forward (and its captured graph) is another one
    Knob("pos", partial(_one_of, "pos", _POSITIONS, "'sinusoid' or 'rope'"),
         applies=partial(_offered, "pos", "positions",
                         "has no position encoding to choose (the knob is for the Transformer models)"),
         default="sinusoid", fixes="model", token="pos={}", sparse=True,
         cli=dict(choices=_POSITIONS,
                  help="position encoding of a Transformer job: rope rotates Q and K inside the self-attention "
                       "kernels (rotary embeddings, pairs (j, j + 32), base 10000) in place of the additive "
                       "sinusoid table; other models reject it; default sinusoid")),
)}

STRUCTURAL = tuple(k for k in KNOBS.values() if k.fixes)


def check_knob(name: str, model: str, v):
    """The value a job of ``model`` runs knob ``name`` with (the knob's
    default when ``v`` is None); ValueError for a value that is not legal, or
    that a job of this model cannot run with."""
    k = KNOBS[name]
    if v is None:
        return k.default
    v = k.value(v)
    if k.applies is not None:
        k.applies(model, v)
    return v


check_cardinality = partial(check_knob, "cardinality")
check_se_ratio = partial(check_knob, "se_ratio")
check_pos = partial(check_knob, "pos")


def check_together(values: Dict[str, Any]) -> None:
    """The rules between knobs (``values``: name -> checked value or None);
    ValueError for a combination that is not supported. (A rule between a
    knob and the model, such as opt_dtype "factored" on a model that is not
    an adam one, is the row's ``applies``.)"""
    if values.get("trust_ratio") is not None:
        if values.get("opt_dtype") in ("bf16", "q8"):
            raise ValueError(f"trust_ratio with opt_dtype={values['opt_dtype']!r} is not supported: LAMB's second "
                             "pass would take the weights from the rounded moments")
        if values.get("opt_dtype") == "factored":
            raise ValueError("trust_ratio with opt_dtype='factored' is not supported: LAMB's ratio is "
                             "defined over Adam's update")


def check_sharded(values: Dict[str, Any]) -> None:
    """ValueError when one of ``values`` (name -> value) is not supported on a
    multi-GPU gang under ddp_shard. The caller knows whether it has one."""
    for name, v in values.items():
        k = KNOBS[name]
        if k.sharded is None or v is None or v == k.default:
            continue
        what = f"{name}={v!r}" if isinstance(k.sharded, dict) else name
        why = k.sharded[v] if isinstance(k.sharded, dict) else k.sharded
        raise ValueError(f"{what} with ddp_shard is not supported: {why}")


def wire(values: Dict[str, Any]) -> Dict[str, Any]:
    """The knob keys of a spool request or a start action: every value that
    is set, null for an always-written knob that is off, nothing for a sparse
    one. TypeError for a name that is not a knob."""
    unknown = sorted(set(values) - set(KNOBS))
    if unknown:
        raise TypeError(f"unknown per-job knob(s) {unknown} (known: {list(KNOBS)})")
    return {k.name: values.get(k.name) for k in KNOBS.values()
            if values.get(k.name) is not None or not k.sparse}
