"""What the Python front of the capture plans says and does, without a GPU: the cases of tests/test_python_front.py and the recorder of
its fixture, tests/golden/python_front.json.

    python tests/python_front_cases.py --record [TREE] > tests/golden/python_front.json

TREE is the checkout whose wayverb_amd/ and tools/ are recorded (default: this one; it needs its libwayverb_amd.so, for the filter
designs).  The fixture was recorded from the commit BEFORE the front's copies were folded (profiles/r21/README.md), so it pins that
the fold changed no sentence, no order of two faults, no argument handed on and no byte handed to the library.

Four groups.  (a) the six *_plan_arguments functions over a mesh stand-in: what a valid dict becomes, and what every fault, and every
ordered pair of two faults in one dict, is answered with.  (b) canonical's refusals, and which set_* / fetch_* it and
impulse_response() call with what, against a recording stand-in for the engine.  (c) the Engine's plan wrappers against a stand-in
library that records the bytes it is handed.  (d) tools/impulse_response.py's refusals, as a child process.

The fixture holds the distinct answers once, and the cases as indices into them.  A group of pairs is a table: answer[i][j] is what
fault i followed by fault j gets (i == j: that fault alone).  Floats are written with float.hex, arrays as dtype, shape and SHA-256."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import types
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "python_front.json")

# The leading words of every sentence wayverb_amd/simulation.py raises as a ValueError and tools/impulse_response.py hands to
# ap.error, grepped out of the commit the fixture was recorded from.  Every one of them is in some recorded answer ...
SENTENCES = [
    "intensity=dict(plane=", "intensity: every must be", "intensity: plane z=",
    "arrival=dict(plane=", "arrival: every must be", "arrival: plane z=", "arrival: bands holds", "arrival: lag is",
    "lateral=dict(plane=", "lateral: every must be", "lateral: edges_ms begins", "lateral: plane z=",
    "modulation=dict(plane=", "modulation: every must be", "modulation: bands_hz holds", "modulation: freqs_hz holds", "modulation: plane z=",
    "modulation maps are accumulated", "lateral maps are accumulated", "arrival maps are accumulated", "intensity bins are accumulated",
    "decay bins are accumulated", "snapshots are taken", "a spectrum is accumulated", "a spectrum plan and a snapshot plan",
    "spectrum: freqs_hz=[...] is required", "spectrum: period must be", "is not a frequency", "Hz is outside 0 ..",
    "this VoxelsAndMesh carries no surface absorptions", "no receivers",
    "--snapshots: single-band runs only", "--snapshots takes z=", "--spectrum: single-band runs without", "--spectrum-plane takes z=",
    "--decay-map: single-band runs without", "--decay-map takes z=", "--decay-every must be", "--decay-bands takes octave centres", "--decay-bands: 1 .. 8",
    "--intensity-map: single-band runs without", "--intensity-plane takes z=", "--intensity-every must be",
    "--clarity-map: single-band runs without", "--arrival-plane takes z=", "--arrival-every must be", "--clarity-bands takes 1 .. 8",
    "--clarity-bands goes with",
    "--lateral-map: single-band runs without", "--lateral-plane takes z=", "--lateral-every must be",
    "--modulation-map: single-band runs without", "--modulation-map takes z=", "--modulation-bands takes octave centres", "--modulation-bands: 1 .. 8",
    "several --receiver: single-band runs without",
]
# ... but these.  Three are said only once a scene has been voxelised on a GPU: the GPU tests' business.  Two are never said: a multi-band
# bundle beside one of these flags is refused earlier in the same run, by the flag's own "single-band runs without ..." sentence.
SENTENCES_BEHIND_A_GPU = ["scene uses %d surfaces", "--spectrum-plane: z=%g m is outside", "--decay-map: z=%g m is outside"]
SENTENCES_NEVER_REACHED = ["--intensity-map, --clarity-map, --lateral-map: single-band runs only", "--modulation-map: single-band runs only"]


def sha(data):
    return hashlib.sha256(data).hexdigest()


def canon(v):
    """A value as the fixture holds it: ints as they are, floats by float.hex, arrays as dtype, shape and digest."""
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "shape": list(v.shape), "sha256": sha(np.ascontiguousarray(v).tobytes())}
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, dict):
        return {str(k): canon(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    if callable(v):
        return "<callable>"
    raise TypeError("no canonical form for %r" % (v,))


def answer(call):
    """What a call is answered with: {"returns": ...} or {"raises": type, "says": sentence}, and the warnings on the way if any."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            out = {"returns": canon(call())}
        except Exception as e:   # noqa: BLE001  (whatever it is, is the record)
            out = {"raises": type(e).__name__, "says": str(e)}
    if caught:
        out["warnings"] = [str(w.message) for w in caught]
    return out


def pair_table(faults, call):
    """{"faults": names, "answer": [[...]]}: answer[i][j] is call() of the base with fault i, then fault j, applied."""
    names = list(faults)
    return {"faults": names, "answer": [[call([faults[a]] if a == b else [faults[a], faults[b]]) for b in names] for a in names]}


# ---- (a) the *_plan_arguments functions ---------------------------------------------------------------------------------------------
MESH = types.SimpleNamespace(dims=(8, 9, 10), spacing=0.05, min_corner=(-0.1, 0.2, 0.3))
RATES = (8000.0, 12000.0)
BOX = ((1, 2, 3), (4, 3, 2))
Z = 0.3 + 4 * 0.05     # plane 4 of the stand-in


def put(**keys):
    return lambda d: d.update(keys)


def drop(*keys):
    return lambda d: [d.pop(k, None) for k in keys]


PLANE_FAULTS = {"unknown-key": put(colour="red"), "plane-and-box": put(plane=Z, box=BOX), "neither": drop("plane", "box"), "every-0": put(every=0),
                "plane-below": put(plane=0.2), "plane-above": put(plane=0.9)}
RIM_FAULTS = dict(PLANE_FAULTS, **{"plane-on-the-floor": put(plane=0.3), "plane-on-the-ceiling": put(plane=0.75)})
ONSET_FAULTS = {"no-threshold": drop("threshold")}
THRESHOLD_MAP = np.full((1, 9, 8), 2e-4, dtype=np.float32)

# per function: the valid dicts (the first is the base the faults go into) and the faults
ARGUMENTS = {
    "intensity": dict(
        valid={"plane": dict(plane=Z), "box": dict(box=BOX), "every-1": dict(plane=Z, every=1), "every-3": dict(plane=Z, every=3),
               "stride": dict(plane=Z, stride=(1, 2, 1)), "n_bins": dict(plane=Z, n_bins=5), "bin_seconds": dict(plane=Z, bin_seconds=0.004),
               "n_bins-and-bin_seconds": dict(plane=Z, n_bins=5, bin_seconds=0.004, every=3), "first_step": dict(box=BOX, first_step=7)},
        faults=RIM_FAULTS),
    "arrival": dict(
        valid={"plane": dict(plane=Z, threshold=1e-4), "box": dict(box=BOX, threshold=1e-4), "every-1": dict(plane=Z, threshold=1e-4, every=1),
               "every-3": dict(plane=Z, threshold=1e-4, every=3), "floor": dict(plane=0.3, threshold=0.0), "stride": dict(plane=Z, threshold=1e-4, stride=2),
               "early_ms": dict(plane=Z, threshold=1e-4, early_ms=(35.0,)), "threshold_map": dict(plane=Z, threshold=1e-4, threshold_map=THRESHOLD_MAP),
               "first_step": dict(box=BOX, threshold=1e-4, first_step=7)},
        faults=dict(PLANE_FAULTS, **ONSET_FAULTS)),
    "arrival_bands": dict(
        valid={"plane": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0), (177.0, 354.0)]), "box": dict(box=BOX, threshold=1e-4, bands=[(88.0, 177.0)]),
               "every-1": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0)], every=1), "every-3": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0)], every=3),
               "tail": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0)], tail_ms=300.0), "tail-bins": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0)],
                                                                                                              tail_ms=300.0, tail_bin_ms=20.0),
               "lag-0": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0), (177.0, 354.0)], lag=0),
               "lag-group-delay": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0)], lag="group-delay"),
               "early_ms": dict(plane=Z, threshold=1e-4, bands=[(88.0, 177.0)], early_ms=(35.0,), stride=2, first_step=7, threshold_map=THRESHOLD_MAP)},
        faults=dict(PLANE_FAULTS, **ONSET_FAULTS, **{"no-bands": put(bands=[]), "nine-bands": put(bands=[(100.0 + k, 200.0 + k) for k in range(9)]),
                                                     "lo-not-below-hi": put(bands=[(200.0, 200.0)]), "lag-by-name": put(lag="minimum-phase"), "lag-1": put(lag=1)})),
    "lateral": dict(
        valid={"plane": dict(plane=Z, threshold=1e-4), "box": dict(box=BOX, threshold=1e-4), "every-1": dict(plane=Z, threshold=1e-4, every=1),
               "every-3": dict(plane=Z, threshold=1e-4, every=3), "stride": dict(plane=Z, threshold=1e-4, stride=2),
               "edges_ms": dict(plane=Z, threshold=1e-4, edges_ms=(0, 10, 40, 80, 120)), "one-edge": dict(plane=Z, threshold=1e-4, edges_ms=(0,)),
               "threshold_map": dict(plane=Z, threshold=1e-4, threshold_map=THRESHOLD_MAP[:, 1:-1, 1:-1]), "first_step": dict(box=BOX, threshold=1e-4, first_step=7)},
        faults=dict(RIM_FAULTS, **ONSET_FAULTS, **{"edges-not-from-0": put(edges_ms=(5, 80)), "nine-edges": put(edges_ms=tuple(range(0, 90, 10))),
                                                   "no-edges": put(edges_ms=())})),
    "modulation": dict(
        valid={"plane": dict(plane=Z), "box": dict(box=BOX), "every-1": dict(plane=Z, every=1), "every-3": dict(plane=Z, every=3),
               "stride": dict(plane=Z, stride=2), "bands_hz": dict(plane=Z, bands_hz=(63, 125)), "one-band": dict(plane=Z, bands_hz=250.0),
               "freqs_hz": dict(plane=Z, freqs_hz=(1.0, 2.0, 4.0)), "one-freq": dict(plane=Z, freqs_hz=2.0), "first_step": dict(box=BOX, first_step=7),
               "untrusted-band": dict(plane=Z, bands_hz=(1000, 2000)), "aliasing-band": dict(plane=Z, bands_hz=(500, 1000), every=3),
               "untrusted-and-aliasing": dict(plane=Z, bands_hz=(4000,))},
        faults=dict(PLANE_FAULTS, **{"no-bands": put(bands_hz=()), "nine-bands": put(bands_hz=tuple(31.5 * 2 ** k for k in range(9))),
                                     "negative-band": put(bands_hz=(125, -250)), "no-freqs": put(freqs_hz=()),
                                     "seventeen-freqs": put(freqs_hz=tuple(0.5 * k for k in range(1, 18)))})),
    "spectrum": dict(
        valid={"freqs": dict(freqs_hz=[0.0, 100.0, 250.0]), "one-freq": dict(freqs_hz=125.0), "period-1": dict(freqs_hz=[100.0], period=1),
               "period-3": dict(freqs_hz=[100.0, 1300.0], period=3), "box": dict(freqs_hz=[100.0], box=BOX, stride=2, first_step=7),
               "nyquist": dict(freqs_hz=[4000.0])},
        faults={"no-freqs_hz": drop("freqs_hz"), "period-0": put(period=0), "nan": put(freqs_hz=[100.0, float("nan")]),
                "above-nyquist": put(freqs_hz=[100.0, 4100.0]), "above-the-series-nyquist": put(freqs_hz=[1400.0], period=3),
                "negative": put(freqs_hz=[-1.0])}),
}


def plan_arguments(W, name, plan, rate):
    env = W.Environment()
    extra = {"intensity": (env, 0.05), "lateral": (env,)}.get(name, ())
    if name == "spectrum":
        return W.spectrum_plan_arguments(plan, rate)
    return getattr(W, name + "_plan_arguments")(plan, MESH, rate, *extra)


def argument_cases(W):
    out = {}
    for name, spec in ARGUMENTS.items():
        out[name + "/valid"] = {"%s@%d" % (case, rate): answer(lambda: plan_arguments(W, name, dict(plan), rate))
                                for case, plan in spec["valid"].items() for rate in RATES}
        base = next(iter(spec["valid"].values()))

        def faulty(faults):
            plan = dict(base)
            for f in faults:
                f(plan)
            return answer(lambda: plan_arguments(W, name, plan, RATES[0]))
        out[name + "/faults"] = pair_table(spec["faults"], faulty)
    return out


# ---- (b) canonical and impulse_response() -------------------------------------------------------------------------------------------
PLAN_KEYWORDS = ("snapshots", "spectrum", "decay", "intensity", "arrival", "lateral", "modulation")


class RecordingEngine:
    """In place of engine.Engine: every call is written down, a fetch returns its own name."""

    def __init__(self, log, *args, **kwargs):
        self.log = log
        log.append(["Engine", canon(args[1:]), canon(kwargs)])

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.log.append([name, canon(args), canon(kwargs)])
            return (7, 6) if name.endswith("_count") else "what %s returned" % name if name.startswith("fetch_") else None
        return method


@contextlib.contextmanager
def stand_ins(module, **names):
    keep = {k: getattr(module, k) for k in names}
    for k, v in names.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(module, k, v)


def box_scene(W):
    from wayverb_amd import mesh as M
    mesh = M.box_mesh(8, 9, 10, coefficients=np.array([M.flat_coefficients(0.1)], dtype=M.coefficients_dtype))
    vm = W.VoxelsAndMesh(None, None, 0, None, None, mesh, (0, 0, 0))
    sp = mesh.spacing
    return vm, (2 * sp, 4 * sp, 5 * sp), (4 * sp, 4 * sp, 5 * sp)


def plan_dicts(W, vm):
    """One valid dict per plan, decay and arrival also with bands: the nine."""
    rate = W.compute_sample_rate(vm.mesh.spacing, W.Environment().speed_of_sound)
    z, box = 5 * vm.mesh.spacing, ((0, 0, 5), (None, None, 1))
    return {
        "snapshots": dict(snapshots=dict(box=box, period=2, keep=3)),
        "spectrum": dict(spectrum=dict(freqs_hz=[0.0, rate / 16.0], box=box, period=2)),
        "decay": dict(decay=dict(n_bins=3, bin_captures=2, box=box, period=2)),
        "decay-bands": dict(decay=dict(n_bins=3, bin_captures=2, box=box, period=2, bands=[(rate / 64.0, rate / 32.0), (rate / 32.0, rate / 16.0)])),
        "intensity": dict(intensity=dict(plane=z, every=2, n_bins=2)),
        "arrival": dict(arrival=dict(plane=z, threshold=1e-4, early_ms=(0.5,))),
        "arrival-bands": dict(arrival=dict(plane=z, threshold=1e-4, early_ms=(0.5,), bands=[(rate / 64.0, rate / 32.0)], tail_ms=2.0, tail_bin_ms=0.5)),
        "lateral": dict(lateral=dict(plane=z, threshold=1e-4, edges_ms=(0, 0.5))),
        "modulation": dict(modulation=dict(plane=z, bands_hz=(rate / 32.0,), freqs_hz=(rate / 256.0,))),
        "snapshots+decay": dict(snapshots=dict(box=box, period=2), decay=dict(n_bins=3, box=box)),
        "none": {},
    }


def canonical_cases(W):
    out = {}

    def slabbed(keywords):
        return answer(lambda: W.canonical(None, None, None, None, 100.0, 0.6, 0.01, slabs=2, **{k: {} for k in keywords}))
    out["canonical/slabs"] = pair_table({k: k for k in PLAN_KEYWORDS}, slabbed)
    out["canonical/refusals"] = {
        "spectrum+snapshots": answer(lambda: W.canonical(None, None, None, None, 100.0, 0.6, 0.01, spectrum={}, snapshots={})),
        "multiband-without-absorptions": answer(lambda: W.canonical_multiband(types.SimpleNamespace(surface_absorptions=None), None, None, None, 3, 100.0, 0.6, 0.01)),
        "no-receivers": answer(lambda: W.impulse_responses(None, None, None, None, [])),
    }
    vm, source, receiver = box_scene(W)
    env = W.Environment()
    rate = W.compute_sample_rate(vm.mesh.spacing, env.speed_of_sound)

    def sequence(plans, seconds=9.5 / rate):
        log = []

        def run_fast(eng, kind, index, signal, receivers, keep_going=None):
            log.append(["run_fast", canon([kind, index, signal, receivers])])
            return signal.shape[0], np.zeros((signal.shape[0], 7))

        def call():
            with stand_ins(W.E, Engine=lambda *a, **k: RecordingEngine(log, *a, **k), run_fast=run_fast):
                got = W.canonical(vm, source, receiver, env, 100.0, 0.6, seconds, precision="f32", **plans)
            return ["bands of %d" % len(got)] if isinstance(got, list) else ["bands of %d" % len(got[0]), got[1]]
        return dict(answer(call), calls=log)
    out["canonical/calls"] = {name: sequence(plans) for name, plans in plan_dicts(W, vm).items()}

    def front(plans):
        """impulse_response(): which plans canonical gets, from dicts and from functions of the mesh, and how many members come back."""
        log = []

        def canonical(vm_, source_, receiver_, environment, cutoff, usable_portion, simulation_time, precision, device, **given):
            log.append(["canonical", canon(given)])
            return (["bands"], "what was taken") if given else ["bands"]

        def call():
            with stand_ins(W, compute_voxels_and_mesh=lambda *a, **k: vm, canonical=canonical), stand_ins(W.P, postprocess=lambda *a, **k: "audio"):
                got = W.impulse_response(None, None, None, source, receiver, **plans)
            return [g if isinstance(g, str) else type(g).__name__ for g in got]
        return dict(answer(call), calls=log)
    fronts = dict(plan_dicts(W, vm))
    fronts["functions-of-the-mesh"] = dict(snapshots=lambda mesh: dict(box=((0, 0, 0), mesh.dims), period=mesh.dims[0]),
                                           decay=lambda mesh, r: dict(n_bins=mesh.dims[1], bin_captures=int(r) // 1000))
    fronts["spectrum-of-the-mesh"] = dict(spectrum=lambda mesh: dict(freqs_hz=[float(mesh.dims[2])]))
    fronts["spectrum+snapshots"] = dict(spectrum={}, snapshots={})
    out["impulse_response/calls"] = {name: front(plans) for name, plans in fronts.items()}
    return out


# ---- (c) the Engine's plan wrappers -------------------------------------------------------------------------------------------------
class RecordingLibrary:
    """In place of libwayverb_amd.so: every wv_* returns 0 and writes down its name and arguments -- behind a byref the bytes of the
    structure, at a pointer the bytes the case says lie there (or, for a fetch, which array it is), integers as they are."""

    def __init__(self):
        self.calls = []
        self.lengths = []      # the bytes behind the pointer arguments of the next call, in order
        self.arrays = None     # a fetch: filled with (pointer, ...) to be matched against what comes back

    def __getattr__(self, name):
        def fn(*args):
            seen, lengths = [], list(self.lengths)
            for i, a in enumerate(args):
                if hasattr(a, "_obj"):
                    if isinstance(a._obj, C.c_uint64):      # a result word: give it a value of its own
                        a._obj.value = 50 - i
                        seen.append("-> %d" % (50 - i))
                    else:
                        seen.append({"struct": type(a._obj).__name__, "sha256": sha(bytes(a._obj))})
                elif isinstance(a, C.c_void_p):
                    if self.arrays is not None:
                        self.arrays.append(a.value)
                        seen.append("array %d" % (len(self.arrays) - 1))
                    else:
                        seen.append({"pointer": sha(C.string_at(a, lengths.pop(0)))})
                else:
                    seen.append(canon(a))
            self.calls.append([name] + seen)
            return 0
        return fn


def stand_in_engine(E):
    eng = E.Engine.__new__(E.Engine)
    eng.lib, eng.h, eng.mesh = RecordingLibrary(), None, types.SimpleNamespace(dims=(8, 9, 10))
    eng._plan_state()
    return eng


def plan_attributes(eng):
    """The plan state that is not None or False ("engine/plan state" holds which names a fresh engine has)."""
    return {k: canon(v) for k, v in sorted(vars(eng).items()) if (k.endswith("_shape") or k == "decay_banded") and v not in (None, False)}


def sections(k, s):
    return np.arange(k * s * 5, dtype=np.float64).reshape(k, s, 5) / 7.0


FREQS = [0.0, 0.125, 0.25]
CONSTANTS = dict(spacing=0.05, sample_rate=8000.0, ambient_density=1.2)
# per setter: the arguments it cannot do without, every keyword given, the bytes behind its pointers, and the arguments of the stop call
SETTERS = {
    "set_snapshots": dict(needs={}, given=dict(first_step=5, period=3, keep=4), pointers=lambda kw: [], stop=dict(box=None)),
    "set_spectrum": dict(needs=dict(freqs=FREQS), given=dict(first_step=5, period=3), pointers=lambda kw: [24], stop=dict(freqs=None)),
    "set_decay": dict(needs=dict(n_bins=6), given=dict(bin_captures=4, first_step=5, period=3), pointers=lambda kw: [], stop=dict(n_bins=None)),
    "set_decay bands": dict(needs=dict(n_bins=6, bands=sections(2, 3)), given=dict(bin_captures=4, first_step=5, period=3), pointers=lambda kw: [240],
                            stop=dict(n_bins=None)),
    "set_intensity": dict(needs=dict(n_bins=6, **CONSTANTS), given=dict(bin_captures=4, first_step=5, period=3), pointers=lambda kw: [],
                          stop=dict(n_bins=None)),
    "set_arrival": dict(needs=dict(edges=[0, 4, 9]), given=dict(threshold=1e-3, first_step=5, period=3, threshold_map="of the box"),
                        pointers=lambda kw: [kw["threshold_map"].nbytes] if kw.get("threshold_map") is not None else [], stop=dict(edges=None)),
    "set_lateral": dict(needs=dict(edges=[0, 4, 9], **CONSTANTS), given=dict(threshold=1e-3, first_step=5, period=3, threshold_map="of the box"),
                        pointers=lambda kw: [kw["threshold_map"].nbytes] if kw.get("threshold_map") is not None else [], stop=dict(edges=None)),
    "set_modulation": dict(needs=dict(freqs=FREQS, bands=sections(2, 3)), given=dict(first_step=5, period=3), pointers=lambda kw: [24, 240],
                           stop=dict(freqs=None, bands=None)),
    "set_arrival_bands": dict(needs=dict(edges=[0, 4, 9], bands=sections(2, 3)),
                              given=dict(threshold=1e-3, tail=(5, 12, 3), lag=[2, 7], first_step=5, period=3, threshold_map="of the box", reserved=0),
                              pointers=lambda kw: ([kw["threshold_map"].nbytes] if kw.get("threshold_map") is not None else []) + [240],
                              stop=dict(edges=None, bands=None)),
}
BOXES = {"every-keyword": dict(box=((1, 2, 3), (4, 3, 2)), stride=(1, 2, 1)), "defaults": {}, "box-mesh": dict(box="mesh"),
         "open-extents": dict(box=((1, 2, 3), (None, 4, None))), "stride-2": dict(box=((1, 1, 1), (5, 6, 7)), stride=2),
         "stride-per-axis": dict(box=((1, 1, 1), (5, 6, 7)), stride=(1, 2, 3)), "stride-0": dict(box=((1, 1, 1), (5, 6, 7)), stride=0),
         "extent-0": dict(box=((1, 1, 1), (0, 3, 2)))}


def taken_shape(box, stride):
    """[nz, ny, nx] of BOXES' every-keyword entry -- the shape a threshold map of it has."""
    return tuple(-(-e // s) for e, s in zip(box[1], stride))[::-1]


def setter_call(E, name, kwargs, lengths=None):
    eng = stand_in_engine(E)
    eng.lib.lengths = SETTERS[name]["pointers"](kwargs) if lengths is None else lengths
    out = answer(lambda: getattr(eng, name.split()[0])(**kwargs))
    return dict(out, attributes=plan_attributes(eng), calls=digests(eng.lib.calls))


def digests(calls):
    """[[wv_name, argument, ...]] -> [[wv_name, one digest over its arguments]]: a setter's are digests and integers already."""
    return [[call[0], sha(json.dumps(call[1:], sort_keys=True).encode())] for call in calls]


def engine_cases(E):
    out = {}
    for name, spec in SETTERS.items():
        cases = {}
        for case, box in BOXES.items():
            kwargs = dict(spec["needs"], **box)
            if case == "every-keyword":
                kwargs.update(spec["given"])
                if "threshold_map" in kwargs:
                    shape = taken_shape(box["box"], box["stride"])
                    kwargs["threshold_map"] = np.linspace(1e-4, 1e-3, int(np.prod(shape)), dtype=np.float32).reshape(shape)
            cases[case] = setter_call(E, name, kwargs)
        eng = stand_in_engine(E)     # set, then stop: what is forgotten
        eng.lib.lengths = spec["pointers"](spec["needs"])
        getattr(eng, name.split()[0])(**spec["needs"])
        eng.lib.calls.clear()
        stopped = answer(lambda: getattr(eng, name.split()[0])(**spec["stop"]))
        cases["stop"] = dict(stopped, attributes=plan_attributes(eng), calls=digests(eng.lib.calls))
        out["engine/" + name] = cases
    out["engine/plan state"] = {"fresh": answer(lambda: {k: v for k, v in sorted(vars(stand_in_engine(E)).items()) if k not in ("lib", "h", "mesh")})}
    # (one lag for nine bands is the library's to refuse: eight lags go over)
    out["engine/set_arrival_bands"]["nine-bands-one-lag"] = setter_call(E, "set_arrival_bands", dict(edges=[0, 4], bands=sections(9, 1), lag=1), lengths=[360])
    bad_map = np.zeros((2, 3, 5), dtype=np.float32)
    box = dict(box=((1, 2, 3), (4, 3, 2)))
    out["engine/refusals"] = {
        "set_arrival 17 edges": setter_call(E, "set_arrival", dict(edges=list(range(17)))),
        "set_lateral 9 edges": setter_call(E, "set_lateral", dict(edges=list(range(9)))),
        "set_arrival_bands 17 edges": setter_call(E, "set_arrival_bands", dict(edges=list(range(17)), bands=sections(2, 3))),
        "set_decay bands [2][5]": setter_call(E, "set_decay", dict(n_bins=6, bands=np.zeros((2, 5)))),
        "set_decay bands [2][3][6]": setter_call(E, "set_decay", dict(n_bins=6, bands=np.zeros((2, 3, 6)))),
        "set_modulation bands [2][3][6]": setter_call(E, "set_modulation", dict(freqs=FREQS, bands=np.zeros((2, 3, 6)))),
        "set_arrival_bands bands [2][3][6]": setter_call(E, "set_arrival_bands", dict(edges=[0, 4], bands=np.zeros((2, 3, 6)))),
        "set_arrival_bands bands and 17 edges": setter_call(E, "set_arrival_bands", dict(edges=list(range(17)), bands=np.zeros((2, 3, 6)))),
        "set_arrival map": setter_call(E, "set_arrival", dict(edges=[0, 4], threshold_map=bad_map, **box)),
        "set_lateral map": setter_call(E, "set_lateral", dict(edges=[0, 4], threshold_map=bad_map, **box, **CONSTANTS)),
        "set_arrival_bands map": setter_call(E, "set_arrival_bands", dict(edges=[0, 4], bands=sections(2, 3), threshold_map=bad_map, **box)),
        "set_arrival_bands 3 lags of 2 bands": setter_call(E, "set_arrival_bands", dict(edges=[0, 4], bands=sections(2, 3), lag=[1, 2, 3])),
        "set_arrival_bands 9 lags": setter_call(E, "set_arrival_bands", dict(edges=[0, 4], bands=sections(9, 1), lag=list(range(9)))),
        "set_arrival_bands lags and map": setter_call(E, "set_arrival_bands", dict(edges=[0, 4], bands=sections(2, 3), lag=[1], threshold_map=bad_map, **box)),
    }

    def fetch(method, attributes, *args, **kwargs):
        eng = stand_in_engine(E)
        for k, v in attributes.items():
            setattr(eng, k, v)
        eng.lib.arrays = []
        got = getattr(eng, method)(*args, **kwargs)
        flat = []

        def walk(v, path):
            if isinstance(v, np.ndarray):
                at = [i for i, p in enumerate(eng.lib.arrays) if p == v.ctypes.data]
                flat.append([path, str(v.dtype), list(v.shape), at[0] if at and v.size else None])
            elif isinstance(v, dict):
                [walk(x, path + "." + k) for k, x in v.items()]
            elif isinstance(v, tuple):
                [walk(x, path + "[%d]" % i) for i, x in enumerate(v)]
            else:
                flat.append([path, canon(v)])
        walk(got, "")
        return dict(returns=flat, calls=eng.lib.calls)
    shape4, shape5 = (3, 2, 4, 5), (2, 3, 2, 4, 5)
    out["engine/fetches"] = {
        "fetch_snapshots": fetch("fetch_snapshots", dict(snapshot_shape=(2, 4, 5))),
        "fetch_snapshots 3 from 1": fetch("fetch_snapshots", dict(snapshot_shape=(2, 4, 5)), 1, 3),
        "fetch_snapshots from 1": fetch("fetch_snapshots", dict(snapshot_shape=(2, 4, 5)), first=1),
        "fetch_spectrum": fetch("fetch_spectrum", dict(spectrum_shape=shape4)),
        "fetch_decay": fetch("fetch_decay", dict(decay_shape=shape4)),
        "fetch_decay of a banded plan": fetch("fetch_decay", dict(decay_shape=shape5, decay_banded=True)),
        "fetch_decay banded=False of a banded plan": fetch("fetch_decay", dict(decay_shape=shape5, decay_banded=True), banded=False),
        "fetch_decay banded=True of a plain plan": fetch("fetch_decay", dict(decay_shape=shape4), banded=True),
        "fetch_intensity": fetch("fetch_intensity", dict(intensity_shape=(4,) + shape4)),
        "fetch_intensity_velocity": fetch("fetch_intensity_velocity", dict(intensity_shape=(4,) + shape4)),
        "fetch_arrival": fetch("fetch_arrival", dict(arrival_shape=shape4)),
        "fetch_lateral": fetch("fetch_lateral", dict(lateral_shape=(10,) + shape4)),
        "fetch_modulation": fetch("fetch_modulation", dict(modulation_shape=shape5)),
        "fetch_arrival_bands": fetch("fetch_arrival_bands", dict(arrival_bands_shape=shape5)),
    }
    fetches = ("fetch_snapshots", "fetch_spectrum", "fetch_decay", "fetch_intensity", "fetch_intensity_velocity", "fetch_arrival", "fetch_lateral",
               "fetch_modulation", "fetch_arrival_bands")
    out["engine/fetches without a plan"] = {m: fetch(m, {}) for m in fetches}
    out["engine/counts"] = {m: fetch(m, {}) for m in ("snapshot_count", "spectrum_count", "decay_count", "intensity_count", "arrival_count", "lateral_count",
                                                      "modulation_count", "arrival_bands_count")}
    return out


# ---- (d) the tool -------------------------------------------------------------------------------------------------------------------
PLAN_FLAGS = {"--snapshots": ["z=1,every=2"], "--spectrum": ["100"], "--decay-map": [], "--intensity-map": [], "--clarity-map": [], "--lateral-map": [],
              "--modulation-map": []}
MALFORMED = {
    "--snapshots with wrong keys": ["--snapshots", "z=1,each=2"],
    "--spectrum-plane": ["--spectrum", "100", "--spectrum-plane", "1.5"],
    "--decay-map": ["--decay-map", "1.5"],
    "--intensity-plane": ["--intensity-map", "--intensity-plane", "1.5"],
    "--arrival-plane": ["--clarity-map", "--arrival-plane", "y=1.5"],
    "--lateral-plane": ["--lateral-map", "--lateral-plane", "1.5"],
    "--modulation-map": ["--modulation-map", "1.5"],
    "--decay-every 0": ["--decay-map", "--decay-every", "0"],
    "--intensity-every 0": ["--intensity-map", "--intensity-every", "0"],
    "--arrival-every 0": ["--clarity-map", "--arrival-every", "0"],
    "--lateral-every 0": ["--lateral-map", "--lateral-every", "0"],
    "--modulation-every 0": ["--modulation-map", "--modulation-every", "0"],
    "--decay-bin-ms 0": ["--decay-map", "--decay-bin-ms", "0"],
    "--decay-bin-ms nan": ["--decay-map", "--decay-bin-ms", "nan"],
    "--intensity-bin-ms -1": ["--intensity-map", "--intensity-bin-ms", "-1"],
    "--arrival-threshold -1": ["--clarity-map", "--arrival-threshold", "-1"],
    "--arrival-threshold inf": ["--clarity-map", "--arrival-threshold", "inf"],
    "--arrival-threshold nan": ["--clarity-map", "--arrival-threshold", "nan"],
    "--lateral-threshold -1": ["--lateral-map", "--lateral-threshold", "-1"],
    "--lateral-threshold inf": ["--lateral-map", "--lateral-threshold", "inf"],
    "--decay-bands by name": ["--decay-map", "--decay-bands", "low,high"],
    "--decay-bands nine": ["--decay-map", "--decay-bands", "1,2,3,4,5,6,7,8,9"],
    "--decay-bands negative": ["--decay-map", "--decay-bands", "125,-250"],
    "--clarity-bands nine": ["--clarity-map", "--clarity-bands", "1,2,3,4,5,6,7,8,9"],
    "--clarity-bands zero": ["--clarity-map", "--clarity-bands", "0"],
    "--clarity-bands without --clarity-map": ["--clarity-bands", "125"],
    "--modulation-bands by name": ["--modulation-map", "--modulation-bands", "low"],
    "--modulation-bands nine": ["--modulation-map", "--modulation-bands", "1,2,3,4,5,6,7,8,9"],
    "--modulation-bands negative": ["--modulation-map", "--modulation-bands", "-125"],
    "--sti-rest without a colon": ["--modulation-map", "--sti-rest", "1000"],
    "--sti-rest by name": ["--modulation-map", "--sti-rest", "1000:good"],
    "--decay-map and --decay-every 0": ["--decay-map", "1.5", "--decay-every", "0"],
    "--lateral-plane and --lateral-every 0": ["--lateral-map", "--lateral-plane", "1.5", "--lateral-every", "0"],
    # a z= whose number does not parse is converted behind the flag's other checks: theirs is the refusal
    "--decay-map z=abc and --decay-every 0": ["--decay-map", "z=abc", "--decay-every", "0"],
    "--intensity-plane z=abc and --intensity-bin-ms 0": ["--intensity-map", "--intensity-plane", "z=abc", "--intensity-bin-ms", "0"],
    "--arrival-plane z=abc and --arrival-threshold -1": ["--clarity-map", "--arrival-plane", "z=abc", "--arrival-threshold", "-1"],
    "--lateral-plane z=abc and --lateral-every 0": ["--lateral-map", "--lateral-plane", "z=abc", "--lateral-every", "0"],
    "--modulation-map z=abc and --modulation-every 0": ["--modulation-map", "z=abc", "--modulation-every", "0"],
}
# tests/golden/sample.way is a multi-band project (waveguide mode "multiple", 3 bands): every plan flag beside it is refused before an
# engine exists.  (--way gives the run the bundle's one receiver, so "several --receiver" cannot be said of a multi-band run.)
WAY = ["--way", os.path.join("tests", "golden", "sample.way")]


def tool_cases(root):
    tool = os.path.join(root, "tools", "impulse_response.py")

    def run(arguments):
        p = subprocess.run([sys.executable, tool] + arguments, capture_output=True, text=True, timeout=120, cwd=root,
                           env=dict(os.environ, COLUMNS="80"))      # (argparse folds --help to the terminal's width)
        return p

    def refusal(arguments):
        p = run(arguments)
        lines = p.stderr.strip().splitlines()
        return {"exit": p.returncode, "says": lines[-1].replace(os.path.basename(tool), "impulse_response.py") if lines else ""}
    jobs = {}
    for a, a_value in PLAN_FLAGS.items():
        for b, b_value in PLAN_FLAGS.items():
            if a != b:
                jobs["pairs/%s %s" % (a, b)] = [a] + a_value + [b] + b_value
        jobs["receivers/" + a] = ["--receiver", "8", "20", "1.2", "--receiver", "4", "12", "1.2", a] + a_value
        jobs["multiband/" + a] = WAY + [a] + a_value
        jobs["multiband/%s and a second --receiver" % a] = WAY + ["--receiver", "8", "20", "1.2", "--receiver", "4", "12", "1.2", a] + a_value
    for name, arguments in MALFORMED.items():
        jobs["malformed/" + name] = arguments
    with ThreadPoolExecutor(8) as pool:
        done = dict(zip(jobs, pool.map(refusal, jobs.values())))
    out = {}
    for name, got in done.items():
        group, case = name.split("/", 1)
        out.setdefault("tool/" + group, {})[case] = got
    out["tool/help"] = {"--help": {"exit": run(["--help"]).returncode, "sha256": sha(run(["--help"]).stdout.encode())}}
    assert all("single-band runs" in got["says"] for got in out["tool/multiband"].values()), out["tool/multiband"]   # (the bundle IS multi-band)
    return out


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def record(root=ROOT):
    """{group: {case: answer}} of the tree at `root` (whose wayverb_amd must be the one imported)."""
    sys.path.insert(0, root)
    from wayverb_amd import engine as E
    from wayverb_amd import simulation as W
    assert os.path.dirname(os.path.dirname(os.path.abspath(W.__file__))) == os.path.abspath(root), W.__file__
    out = {}
    for part in (argument_cases(W), canonical_cases(W), engine_cases(E), tool_cases(root)):
        out.update(part)
    return out


def cases_of(groups):
    """{group: {case: answer}} -> [(name, answer)], a pair table spread into its cases."""
    flat = []
    for group, cases in groups.items():
        if "faults" in cases and "answer" in cases:
            names = cases["faults"]
            flat += [("%s/%s" % (group, a) if a == b else "%s/%s then %s" % (group, a, b), cases["answer"][i][j])
                     for i, a in enumerate(names) for j, b in enumerate(names)]
        else:
            flat += [("%s/%s" % (group, case), got) for case, got in cases.items()]
    return flat


def pack(groups):
    """The fixture: the distinct answers once, the cases as indices into them."""
    answers = []

    def index(got):
        text = json.dumps(got, sort_keys=True)
        if text not in answers:
            answers.append(text)
        return answers.index(text)
    packed = {}
    for group, cases in groups.items():
        if "faults" in cases and "answer" in cases:
            packed[group] = {"faults": cases["faults"], "answer": [[index(got) for got in row] for row in cases["answer"]]}
        else:
            packed[group] = {case: index(got) for case, got in cases.items()}
    return {"numpy": np.__version__, "answers": [json.loads(a) for a in answers], "cases": packed}


def unpack(fixture):
    answers = fixture["answers"]
    groups = {}
    for group, cases in fixture["cases"].items():
        if "faults" in cases and "answer" in cases:
            groups[group] = {"faults": cases["faults"], "answer": [[answers[i] for i in row] for row in cases["answer"]]}
        else:
            groups[group] = {case: answers[i] for case, i in cases.items()}
    return groups


def write(fixture, out):
    """One answer and one group a line: small, and a diff shows which."""
    out.write('{"numpy": %s,\n"answers": [\n' % json.dumps(fixture["numpy"]))
    out.write(",\n".join(json.dumps(a, sort_keys=True) for a in fixture["answers"]))
    out.write('\n],\n"cases": {\n')
    out.write(",\n".join("%s: %s" % (json.dumps(g), json.dumps(c)) for g, c in fixture["cases"].items()))
    out.write("\n}}\n")


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    write(pack(record(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT)), sys.stdout)
