"""The full training state of the training entries as ONE file, and its host logic (--save_state_every / --resume).

A state is one ``torch.save`` dict whose tensors are all on the CPU and whose other values are ints, floats, strs, None,
lists and dicts, so that ``torch.load(path, map_location="cpu", weights_only=True)`` reads it: no pickled NumPy array,
namespace or class.  Nothing here touches a device: the helpers take state_dicts (the copy to the CPU is ``Tensor.cpu``)."""
import os
import random
import re

import numpy as np
import torch

FORMAT = 1
KEYS = ("format", "epoch", "steps_done", "flags", "model", "optimizer", "queue", "key_encoder", "swav", "rng")
RNG_KEYS = ("numpy", "python", "torch_cpu", "device", "view_run", "view_source")

# every option that determines the trajectory: a resumed run must repeat them
TRAJECTORY_FLAGS = ("batchSize", "num_crop", "SAMPLE_NUM", "INPUT_FEATURE_NUM", "branch_choose", "dataset", "split", "full_train",
                    "synthetic", "view_rng", "steps_per_epoch", "max_steps_per_epoch", "learning_rate", "precision",
                    "group_radius", "fps_reorder", "knn_K", "sample_num_level1", "sample_num_level2", "ball_radius", "ball_radius2",
                    "Num_Class", "swa_if", "cld_if", "loss_normalize", "loss_temperature", "loss_mask", "neg_queue", "key_encoder",
                    "key_momentum", "adamw_decay", "clip_grad_norm", "lr_schedule", "warmup_steps", "lr_decay_epochs", "lr_min",
                    "view_kinds", "jitter_sigma", "jitter_clip", "rot_range", "scale_lo", "scale_hi", "tilt_angle",
                    "label_fraction", "label_seed", "class_positives",
                    "optim", "sgd_momentum", "sgd_nesterov", "sgd_weight_decay", "lars_eta")

# the optimizer-recipe flags and the view-recipe flags came after the first states were written: a state without them ran with
# the recipe off / with the reference's ten views at its strengths, which is what these defaults (the parser's) say; so did the
# labelled fraction of the class-aware loss mask (every label, seed 0: the mask itself did not exist) and the weight of
# class-mates as extra positives (0: off).  Every other flag must be in the file, but for OPTIMIZER_FLAG_DEFAULTS below.
LATER_FLAG_DEFAULTS = {"adamw_decay": 0.0, "clip_grad_norm": 0.0, "lr_schedule": "step", "warmup_steps": 0, "lr_decay_epochs": 0,
                       "lr_min": 0.0, "view_kinds": "reference", "jitter_sigma": 0.01, "jitter_clip": 0.05, "rot_range": 0.8,
                       "scale_lo": 0.5, "scale_hi": 1.5, "tilt_angle": 0.25, "label_fraction": 1.0, "label_seed": 0,
                       "class_positives": 0.0}

# --optim and the four flags of SGD / LARS (the training entries' own parser, train_flags.add_optimizer_flags): a state without
# them was an Adam run, and a namespace without them (build_parser's: the extraction entries share it) is one too
OPTIMIZER_FLAG_DEFAULTS = {"optim": "adam", "sgd_momentum": 0.9, "sgd_nesterov": 0, "sgd_weight_decay": 0.0, "lars_eta": 0.001}

_STATE_NAME = re.compile(r"^state_(\d+)\.pth$")


class StateUnreadable(RuntimeError):
    """The file is not a readable torch archive (a damaged or foreign file): --resume auto goes on to the next older state."""


def state_path(folder, epoch):
    return os.path.join(folder, "state_%d.pth" % epoch)


# ---- tensors -------------------------------------------------------------------------------------------------------------
def to_cpu(obj):
    """A deep copy with every tensor on the CPU and in storage of its own (FusedAdam.state_dict() shares its moments)."""
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [to_cpu(v) for v in obj]
    return obj


def flag_of(opt, k):
    """The value of trajectory flag `k` in the namespace `opt`; the optimizer's flags read as Adam's where `opt` has none."""
    return getattr(opt, k, OPTIMIZER_FLAG_DEFAULTS[k]) if k in OPTIMIZER_FLAG_DEFAULTS else getattr(opt, k)


def flags_of(opt):
    return {k: flag_of(opt, k) for k in TRAJECTORY_FLAGS}


# ---- generators ----------------------------------------------------------------------------------------------------------
def pack_numpy(st):
    """``RandomState.get_state()`` / ``np.random.get_state()`` -> tensors and scalars (the 624 key words as int64)."""
    name, keys, pos, has_gauss, cached = st
    if name != "MT19937":
        raise ValueError("a NumPy generator of kind %r cannot be stored" % (name,))
    return {"keys": torch.from_numpy(np.asarray(keys, dtype=np.int64).copy()), "pos": int(pos), "has_gauss": int(has_gauss),
            "cached_gaussian": float(cached)}


def unpack_numpy(d):
    return ("MT19937", d["keys"].numpy().astype(np.uint32), int(d["pos"]), int(d["has_gauss"]), float(d["cached_gaussian"]))


def pack_python(st):
    """``random.getstate()`` -> the 625 words as an int64 tensor, the version and gauss_next (a float or None)."""
    version, words, gauss_next = st
    return {"version": int(version), "words": torch.tensor(list(words), dtype=torch.int64), "gauss_next": gauss_next}


def unpack_python(d):
    return (int(d["version"]), tuple(int(w) for w in d["words"].tolist()), d["gauss_next"])


def capture_rng(gen=None, view_run=None, view_source=None):
    """NumPy's global generator (the circle-loss shuffle), Python's ``random``, torch's CPU generator, the entry's device
    generator `gen` and the two ``RandomState`` view generators (either may be None)."""
    return {"numpy": pack_numpy(np.random.get_state()), "python": pack_python(random.getstate()),
            "torch_cpu": torch.get_rng_state().clone(),
            "device": None if gen is None else gen.get_state().cpu().clone(),
            "view_run": None if view_run is None else pack_numpy(view_run.get_state()),
            "view_source": None if view_source is None else pack_numpy(view_source.get_state())}


def apply_rng(rng, gen=None, view_run=None, view_source=None):
    np.random.set_state(unpack_numpy(rng["numpy"]))
    random.setstate(unpack_python(rng["python"]))
    torch.set_rng_state(rng["torch_cpu"])
    for name, target in (("view_run", view_run), ("view_source", view_source)):
        if (rng[name] is None) != (target is None):
            raise RuntimeError("the state %s a %s generator and this run %s" % ("holds" if target is None else "lacks", name,
                                                                                "has none" if target is None else "has one"))
        if target is not None:
            target.set_state(unpack_numpy(rng[name]))
    if gen is not None:
        if rng["device"] is None:
            raise RuntimeError("the state lacks the device generator")
        gen.set_state(rng["device"])


# ---- one state -----------------------------------------------------------------------------------------------------------
def assemble(epoch, steps_done, flags, model, optimizer, step_state, rng):
    """`model`, `optimizer`: state_dicts; `step_state`: ``ContrastiveStep.state_dict()``.  Everything is copied to the CPU."""
    return {"format": FORMAT, "epoch": int(epoch), "steps_done": int(steps_done), "flags": dict(flags),
            "model": to_cpu(model), "optimizer": to_cpu(optimizer), "queue": to_cpu(step_state["queue"]),
            "key_encoder": to_cpu(step_state["key_encoder"]), "swav": to_cpu(step_state["swav"]), "rng": to_cpu(rng)}


def write_atomic(state, path):
    """torch.save to a temporary name in the same folder, then os.replace: `path` is either the old file or the whole new one."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def load_state(path):
    """The state at `path` on the CPU; refuses a format this code does not know and a state with a missing entry (a flag of
    LATER_FLAG_DEFAULTS that the file lacks reads as its default)."""
    try:
        state = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise StateUnreadable("%s does not load as a training state (%s: %s)" % (path, type(e).__name__, e)) from e
    if not isinstance(state, dict) or "format" not in state:
        raise RuntimeError("%s is not a training state (no format entry): --resume takes a state_<epoch>.pth written by "
                           "--save_state_every, not a corr_GL checkpoint" % path)
    if state["format"] != FORMAT:
        raise RuntimeError("%s has state format %r; this code reads format %d" % (path, state["format"], FORMAT))
    missing = [k for k in KEYS if k not in state] + ["rng." + k for k in RNG_KEYS if k not in state.get("rng", {})] \
        + ["flags." + k for k in TRAJECTORY_FLAGS if k not in state.get("flags", {}) and k not in LATER_FLAG_DEFAULTS
           and k not in OPTIMIZER_FLAG_DEFAULTS]
    if missing:
        raise RuntimeError("%s lacks %s" % (path, ", ".join(missing)))
    for k, v in list(LATER_FLAG_DEFAULTS.items()) + list(OPTIMIZER_FLAG_DEFAULTS.items()):
        state["flags"].setdefault(k, v)
    return state


def list_states(folder):
    """[(epoch, path)] of the state_<epoch>.pth files of `folder`, ascending by epoch; temporaries and other files are ignored."""
    if not os.path.isdir(folder):
        return []
    found = [(int(m.group(1)), os.path.join(folder, name)) for name in os.listdir(folder)
             for m in [_STATE_NAME.match(name)] if m]
    return sorted(found)


def find_latest(folder):
    """The state_<epoch>.pth of `folder` with the largest epoch, or None."""
    states = list_states(folder)
    return states[-1][1] if states else None


def prune(folder, keep):
    """Remove all but the `keep` newest states of `folder` (`keep` <= 0: keep all); returns the removed paths."""
    if keep <= 0:
        return []
    gone = [path for _, path in list_states(folder)[:-keep]]
    for path in gone:
        os.remove(path)
    return gone


def check_compatible(saved_flags, opt):
    """Every option that determines the trajectory must equal the saved run's; anything else (nepoch, save_root_dir, log_file,
    graph, prefetch, resident, knn_*, main_gpu, workers, the state flags themselves) may differ."""
    differ = ["--%s %r (the state: %r)" % (k, flag_of(opt, k), saved_flags[k]) for k in TRAJECTORY_FLAGS
              if saved_flags[k] != flag_of(opt, k)]
    if differ:
        raise RuntimeError("the state was written by a run with other options, which would not continue its trajectory: "
                           + "; ".join(differ))
