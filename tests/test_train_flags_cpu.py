"""The flags of the training entries (facl_amd/train_flags.py) against what the code recorded before the step, the replay and
the checks were split out of train_common.py: every parser action and default, and the outcome of the entries' check sequences on
151 command lines (tests/golden/train_flag_*.json) -- and the shape the split is meant to keep."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _parser(entry):
    from facl_amd import train_flags as tf
    return tf.finetune_parser() if entry == "finetune" else tf.build_parser('0')


def _jsonable(v):
    return json.loads(json.dumps(v))


@pytest.mark.parametrize("entry", ["pretrain", "finetune"])
def test_parser_actions_and_defaults_are_the_recorded_ones(entry):
    want = _golden("train_flag_defaults.json")[entry]
    p = _parser(entry)
    rows = sorted(([a.dest, a.default, None if a.type is None else a.type.__name__,
                    None if a.choices is None else list(a.choices), a.help] for a in p._actions), key=lambda r: r[0])
    assert _jsonable(rows) == want["actions"]
    assert _jsonable(vars(p.parse_args([]))) == want["defaults"]


REFUSALS = _golden("train_flag_refusals.json")


def _outcome(entry, argv, world):
    from facl_amd import train_flags as tf
    try:
        if entry == "pretrain":
            tf.check_train_flags(tf.build_parser('0').parse_args(argv), world)
        elif entry == "finetune":
            tf.check_finetune_train_flags(tf.finetune_parser().parse_args(argv), world)
        else:                                                    # one check alone: a refusal no sequence reaches
            getattr(tf, entry)(tf.build_parser('0').parse_args(argv), world)
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None


def test_the_recorded_cases_cover_what_they_claim():
    refused = [r for r in REFUSALS if r["outcome"] is not None]
    assert len(REFUSALS) == 151 and len(refused) == 141
    assert {r["entry"] for r in REFUSALS} == {"pretrain", "finetune", "check_key_flags"}


@pytest.mark.parametrize("n", range(len(REFUSALS)))
def test_check_sequence_outcome_is_the_recorded_one(n):
    r = REFUSALS[n]
    assert _outcome(r["entry"], r["argv"], r["world"]) == r["outcome"], (r["entry"], r["world"], " ".join(r["argv"]))


def test_entries_run_the_check_sequences(monkeypatch):
    """run() and finetune.main() refuse through check_train_flags / check_finetune_train_flags with the launcher's WORLD_SIZE."""
    from facl_amd import cn3d_train_motion_GL, finetune
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match=r"^--neg_queue 6 must be a multiple of --batchSize 4"):
        cn3d_train_motion_GL.main(["--neg_queue", "6", "--batchSize", "4", "--key_encoder", "1", "--key_momentum", "1.0"])
    with pytest.raises(RuntimeError, match=r"^fine-tuning runs on one rank only \(got 2 ranks\)"):
        finetune.main(["--swa_if", "1"])
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(RuntimeError, match=r"^--lr_min 0.1 is the end of --lr_schedule cosine"):
        finetune.main(["--lr_min", "0.1"])


def test_the_individual_checks_stay_importable():
    import facl_amd.train_common as tc
    import facl_amd.train_flags as tf
    from facl_amd import finetune
    for name in ("resident", "view", "knn", "loss", "class_mask", "cluster_id", "proto", "queue", "key", "state", "optim"):
        assert getattr(tc, "check_%s_flags" % name) is getattr(tf, "check_%s_flags" % name)
    for name in ("build_parser", "add_view_recipe_flags", "view_recipe", "optim_recipe", "_check_cosine_span", "OPTIM_FLAGS",
                 "VIEW_RECIPE_FLAGS", "VIEW_RECIPE_DEFAULTS"):
        assert getattr(tc, name) is getattr(tf, name)
    assert finetune.check_finetune_flags is tf.check_finetune_flags and finetune.finetune_parser is tf.finetune_parser


def test_importing_the_flags_imports_no_torch():
    code = "import sys, facl_amd.train_flags; print(sorted(m for m in ('torch', 'facl_amd._lib') if m in sys.modules))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "[]"


def test_a_bare_namespace_gets_the_parser_defaults():
    from types import SimpleNamespace
    from facl_amd import train_flags as tf
    bare = SimpleNamespace()
    o = tf.with_defaults(bare)
    assert vars(bare) == {}                                      # the caller's namespace is not written to
    assert vars(o) == tf.FLAG_DEFAULTS == vars(tf.finetune_parser().parse_args([]))
    assert {k: v for k, v in vars(o).items() if k in vars(tf.build_parser('0').parse_args([]))} == vars(tf.build_parser('0').parse_args([]))
    o = tf.with_defaults(SimpleNamespace(key_momentum=0.5, loss_mask="exclude", not_a_flag=3))
    assert (o.key_momentum, o.loss_mask, o.neg_queue) == (0.5, "exclude", 0) and not hasattr(o, "not_a_flag")


# ---- structure --------------------------------------------------------------------------------------------------------------
def test_the_three_steps_share_one_base_and_one_call():
    from facl_amd.dense import DenseStep
    from facl_amd.finetune import FineTuneStep
    from facl_amd.train_step import ContrastiveStep, TrainStep
    for cls in (ContrastiveStep, FineTuneStep, DenseStep):
        assert issubclass(cls, TrainStep)
    assert not issubclass(FineTuneStep, ContrastiveStep) and not issubclass(DenseStep, ContrastiveStep)
    assert not hasattr(DenseStep, "group") and not hasattr(DenseStep, "grouped")      # grouping is not the dense step's
    defining = [cls.__name__ for cls in (TrainStep, ContrastiveStep, FineTuneStep, DenseStep) if "__call__" in vars(cls)]
    assert defining == ["TrainStep"]
    assert "order" in inspect.signature(TrainStep.__call__).parameters
    shuffles = [cls.__name__ for cls in (TrainStep, ContrastiveStep, FineTuneStep, DenseStep)
                if re.search(r"shuffle|draw_order", inspect.getsource(cls))]
    assert shuffles == ["TrainStep"]


def test_graphed_step_probes_nothing_and_no_default_is_written_twice():
    from facl_amd import train_step
    assert "getattr(" not in inspect.getsource(train_step.GraphedStep)
    for name in ("train_common.py", "train_step.py", "train_flags.py", "finetune.py"):
        with open(os.path.join(ROOT, "facl_amd", name)) as f:
            src = f.read()
        assert not re.search(r"""getattr\(\s*opt\s*,\s*["'][^"']+["']\s*,""", src), name
