"""The five phase entries against the same bad arguments, without a GPU
(include/marlnav.h ``marlnav_ppo_train_phase``, ``_mode``, ``_clipped``,
``_monitored``, ``_shuffled``): a good call of each entry over fake pointers,
one field changed at a time; every entry refuses it with rc -1 and a message
that names the field, before any HIP call. The monitored entry is the
actor's, so it has no critic case; the shuffled entry takes the monitor
arguments with the actor and none with the critic."""
import ctypes
import math

import pytest

import test_adam_cpu as ta

FAKE = ta.FAKE
ENTRIES = ("phase", "mode", "clipped", "monitored", "shuffled")
CLIPPED = ("clipped", "monitored", "shuffled")
CASES = [(e, w) for e in ENTRIES for w in ("actor", "critic")
         if not (e == "monitored" and w == "critic")]


def _good(pkg, which, entry, steps=6, pairs=((0, 3), (3, 5)), batch_size=2):
    """A call of ``entry`` that passes every check: 6 stored steps of 8 envs;
    the contiguous entries cut them at ``pairs``, the shuffled one into
    minibatches of ``batch_size`` steps."""
    d, b, ad, ab, _ = ta._good_update(pkg, which)
    d.num_steps = steps
    flat = [x for p in pairs for x in p]
    monitor = entry == "monitored" or (entry == "shuffled" and which == "actor")
    return {"network": 0 if which == "actor" else 1, "d": d, "b": b,
            "bounds": (ctypes.c_int64 * len(flat))(*flat), "B": len(pairs), "bs": batch_size,
            "E": 2, "ad": ad, "ab": ab, "log": FAKE * 300, "mode": pkg.abi.ADVANTAGE_REFERENCE,
            "max_norm": 0.5, "norm_work": FAKE * 301, "norm_log": FAKE * 302,
            "target_kl": 0.02 if monitor else 0.0, "diag_log": FAKE * 303 if monitor else None,
            "stop": FAKE * 304 if monitor else None, "seed": 7, "counter": FAKE * 305,
            "table": FAKE * 306}


def _call(pkg, entry, a):
    lib = pkg.abi.load_library()
    ref = lambda x: None if x is None else ctypes.byref(x)
    head = (a["network"], ref(a["d"]), ref(a["b"]))
    cut = (a["bounds"], a["B"], a["E"])
    rest = (0.01, 0.001, ref(a["ad"]), ref(a["ab"]), a["log"])
    clip = (a["max_norm"], a["norm_work"], a["norm_log"])
    monitor = (a["target_kl"], a["diag_log"], a["stop"])
    if entry == "phase":
        rc = lib.marlnav_ppo_train_phase(*head, *cut, *rest, None)
    elif entry == "mode":
        rc = lib.marlnav_ppo_train_phase_mode(*head, *cut, *rest, a["mode"], None)
    elif entry == "clipped":
        rc = lib.marlnav_ppo_train_phase_clipped(*head, *cut, *rest, a["mode"], *clip, None)
    elif entry == "monitored":
        rc = lib.marlnav_ppo_train_phase_monitored(*head, *cut, *rest, a["mode"], *clip, *monitor,
                                                   None)
    else:
        rc = lib.marlnav_ppo_train_phase_shuffled(*head, a["bs"], a["E"], *rest, a["mode"], *clip,
                                                  *monitor, a["seed"], a["counter"], a["table"],
                                                  None)
    return rc, lib.marlnav_last_error()


def _refused(pkg, entry, a, *words):
    rc, msg = _call(pkg, entry, a)
    assert rc == -1, (entry, rc, msg)
    for w in words:
        assert w in msg, (entry, msg, w)
    with pytest.raises(RuntimeError):
        pkg.abi.check(rc)


def _change(pkg, which, entry, words, **change):
    """The good call with ``change`` applied: a key of the call's dict, or
    ``struct.field`` as ``struct__field``."""
    a = _good(pkg, which, entry)
    for key, value in change.items():
        if "__" in key:
            obj, field = key.split("__")
            setattr(a[obj], field, value)
        else:
            a[key] = value
    _refused(pkg, entry, a, *words)


@pytest.mark.parametrize("entry,which", CASES)
def test_every_entry_refuses_the_shared_bad_arguments(pkg, entry, which):
    other = _good(pkg, "critic" if which == "actor" else "actor", entry)
    for words, change in (
            ((b"network",), {"network": 2}),
            ((b"dims",), {"d": None}),
            ((b"buffers",), {"b": None}),
            ((b"num_epochs",), {"E": 0}),
            ((b"loss_log", b"NULL"), {"log": None}),
            ((b"loss_log", b"aligned"), {"log": FAKE + 4}),
            ((b"beta2",), {"ad__beta2": 1.0}),
            ((b"state",), {"ab__state": None}),
            ((b"adam table",), {"ad": other["ad"], "ab": other["ab"]}),
            ((b"obs", b"NULL"), {"b__obs": None}),
            ((b"returns", b"NULL"), {"b__returns": None}),
            ((b"work", b"NULL"), {"b__work": None})):
        _change(pkg, which, entry, words, **change)
    # a minibatch of one env row (T * P < 2) is refused as the update calls refuse it
    a = _good(pkg, which, entry, pairs=((0, 1), (1, 5)), batch_size=1)
    a["d"].num_parallel = 1
    _refused(pkg, entry, a, b"fewer than 2 env rows")


@pytest.mark.parametrize("entry,which", [c for c in CASES if c[0] in CLIPPED])
def test_the_clipped_entries_refuse_bad_clip_arguments(pkg, entry, which):
    _change(pkg, which, entry, (b"max_norm",), max_norm=math.nan)
    _change(pkg, which, entry, (b"norm_work", b"aligned"), norm_work=FAKE * 301 + 4)


@pytest.mark.parametrize("entry", ["monitored", "shuffled"])
def test_the_monitored_entries_refuse_bad_monitor_arguments(pkg, entry):
    _change(pkg, "actor", entry, (b"target_kl",), target_kl=0.0)
    _change(pkg, "actor", entry, (b"diag_log", b"NULL"), diag_log=None)
    _change(pkg, "actor", entry, (b"stop", b"aligned"), stop=FAKE * 304 + 4)
