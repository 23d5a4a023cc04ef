"""What the eight capture plans' setters say to a plan with a faulty ARGUMENT: the cases of tests/test_gpu_plan_argument_refusals.py and
the recorder of its fixture, tests/golden/plan_argument_refusals.json.

    python tests/plan_argument_faults.py --record        (on a GPU; rewrites the fixture from the library as built)

The fixture was recorded from the commit BEFORE the setters' shared checks were given one statement (snapshot_plan.h: plan_refusal and
its neighbours), so it pins that the move changed neither a code, nor a sentence, nor which of two simultaneous faults is the one said.

A case is a valid plan on a 12 x 10 x 9 mesh -- the box ((1, 1, 1), (4, 3, 2)), stride 1, 24 nodes -- with one fault applied, or two in
order (the second wins where both touch one argument).  The calls go to the library itself, plan structs filled by hand: the Python
layer refuses some of these on its own, and clamps others.  Per setter the fixture holds the distinct answers once and the cases as
indices into them: `null` where the library took the plan (two faults that undo each other)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_argument_refusals.json")

MESH = (12, 10, 9)
BOX = dict(x0=1, y0=1, z0=1, nx=4, ny=3, nz=2, sx=1, sy=1, sz=1, first_step=0, period=1)
NODES = 24
NAN, INF = float("nan"), float("inf")
CONSTANTS = dict(spacing=0.05, sample_rate=8000.0, ambient_density=1.2)


def bands(n_bands, n_sections):
    b = np.zeros((n_bands, n_sections, 5))
    b[:, :, 0] = 1.0
    b[:, :, 3] = -0.25
    return b


# the valid arguments of every setter: the plan's fields, and what goes beside the plan
BASE = {
    "snapshots": dict(BOX, keep=0),
    "spectrum": dict(BOX, n_freqs=2, freqs=[0.0, 0.125]),
    "decay": dict(BOX, n_bins=3, bin_captures=2),
    "decay_bands": dict(BOX, n_bins=3, bin_captures=2, bands=bands(2, 2)),
    "intensity": dict(BOX, n_bins=3, bin_captures=2, **CONSTANTS),
    "arrival": dict(BOX, n_bins=3, threshold=1e-3, edges=[0, 4, 9], map=None),
    "lateral": dict(BOX, n_bins=3, threshold=1e-3, edges=[0, 4, 9], map=None, **CONSTANTS),
    "modulation": dict(BOX, n_freqs=2, freqs=[0.0, 0.125], bands=bands(2, 2)),
}
KINDS = tuple(BASE)


def put(**fields):
    return lambda a: a.update(fields)


def bad_map(value):
    def fault(a):
        m = np.full(NODES, 1e-3, dtype=np.float32)
        m[NODES - 2] = value
        a["map"] = m
    return fault


def bad_band(n_bands=2, n_sections=2, entry=None, value=None):
    def fault(a):
        b = bands(n_bands, n_sections)
        if entry is not None and b.size:
            b.reshape(-1)[entry] = value
        a["bands"] = b
    return fault


# what every setter can refuse a box and a cadence for: a stride of 0 (and below), a period of 0, a box one node past each face
SHARED = {
    "sx 0": put(sx=0), "sy 0": put(sy=0), "sz -1": put(sz=-1), "period 0": put(period=0),
    "past -x": put(x0=-1), "past -y": put(y0=-1), "past -z": put(z0=-1),
    "past +x": put(x0=9), "past +y": put(y0=8), "past +z": put(z0=8),       # the last node taken is node 12 / 10 / 9 of 0 .. 11 / 9 / 8
    "no nodes": put(ny=0),
}
BINS = {"n_bins 0": put(n_bins=0), "n_bins 4097": put(n_bins=4097), "bin_captures 0": put(bin_captures=0)}
FREQS = {"freq NaN": put(freqs=[0.0, NAN]), "freq -0.1": put(freqs=[-0.1, 0.125]), "freq 0.6": put(freqs=[0.0, 0.6]), "freqs NULL": put(freqs=None)}
BANDS = {
    "n_bands 0": bad_band(n_bands=0), "n_bands 9": bad_band(n_bands=9), "n_sections 0": bad_band(n_sections=0), "n_sections 5": bad_band(n_sections=5),
    "coef inf": bad_band(entry=13, value=INF), "coef -inf": bad_band(entry=0, value=-INF), "coef NaN": bad_band(entry=19, value=NAN),
    "sections NULL": put(bands=None),
}
PHYSICAL = {"spacing 0": put(spacing=0.0), "spacing NaN": put(spacing=NAN), "rate -1": put(sample_rate=-1.0), "rate inf": put(sample_rate=INF),
            "density 0": put(ambient_density=-0.0), "density inf": put(ambient_density=INF)}
FACES = {"face -x": put(x0=0), "face -y": put(y0=0), "face -z": put(z0=0), "face +x": put(x0=8), "face +y": put(y0=7), "face +z": put(z0=7)}
ONSET = {"edges[0] 1": put(edges=[1, 4, 9]), "edges equal": put(edges=[0, 4, 4]), "edges fall": put(edges=[0, 9, 4]),
         "threshold -1": put(threshold=-1.0), "threshold NaN": put(threshold=NAN), "threshold inf": put(threshold=INF),
         "map -1": bad_map(-1.0), "map NaN": bad_map(NAN), "map inf": bad_map(INF)}

FAULTS = {
    "snapshots": dict(SHARED),
    "spectrum": dict(SHARED, **FREQS, **{"n_freqs 0": put(n_freqs=0), "n_freqs 65": put(n_freqs=65)}),
    "decay": dict(SHARED, **BINS),
    "decay_bands": dict(SHARED, **BINS, **BANDS),
    "intensity": dict(SHARED, **BINS, **PHYSICAL, **FACES),
    "arrival": dict(SHARED, **ONSET, **{"n_bins 0": put(n_bins=0), "n_bins 17": put(n_bins=17)}),
    "lateral": dict(SHARED, **ONSET, **PHYSICAL, **FACES, **{"n_bins 0": put(n_bins=0), "n_bins 9": put(n_bins=9)}),
    "modulation": dict(SHARED, **FREQS, **BANDS, **{"n_freqs 0": put(n_freqs=0), "n_freqs 17": put(n_freqs=17)}),
}


def pointer(array):
    return None if array is None else array.ctypes.data_as(C.c_void_p)


def call(eng, kind, args):
    """The setter of `kind` with `args`, on the library itself -> the return code."""
    from wayverb_amd import engine as E
    plan = {"snapshots": E.WvSnapshotPlan, "spectrum": E.WvSpectrumPlan, "decay": E.WvDecayPlan, "decay_bands": E.WvDecayPlan,
            "intensity": E.WvIntensityPlan, "arrival": E.WvArrivalPlan, "lateral": E.WvLateralPlan, "modulation": E.WvModulationPlan}[kind]()
    for name, _ in plan._fields_:
        if name == "edges":
            for k, v in enumerate(args["edges"]):
                plan.edges[k] = v
        elif name in args:
            setattr(plan, name, args[name])
    lib, keep = eng.lib, []    # (keep: the arrays the pointers point into)
    for name in ("freqs", "bands", "map"):
        a = args.get(name)
        keep.append(None if a is None else np.ascontiguousarray(a, dtype=np.float32 if name == "map" else np.float64))
    freqs, sections, threshold_map = keep
    shape = sections.shape[:2] if sections is not None else (2, 2)
    if kind == "snapshots":
        return lib.wv_set_snapshots(eng.h, C.byref(plan))
    if kind == "spectrum":
        return lib.wv_set_spectrum(eng.h, C.byref(plan), pointer(freqs))
    if kind == "decay":
        return lib.wv_set_decay(eng.h, C.byref(plan))
    if kind == "decay_bands":
        return lib.wv_set_decay_bands(eng.h, C.byref(plan), pointer(sections), shape[0], shape[1])
    if kind == "intensity":
        return lib.wv_set_intensity(eng.h, C.byref(plan))
    if kind == "arrival":
        return lib.wv_set_arrival(eng.h, C.byref(plan), pointer(threshold_map))
    if kind == "lateral":
        return lib.wv_set_lateral(eng.h, C.byref(plan), pointer(threshold_map))
    return lib.wv_set_modulation(eng.h, C.byref(plan), pointer(freqs), pointer(sections), shape[0], shape[1])


def stop(eng, kind):
    lib = eng.lib
    rc = {"snapshots": lambda: lib.wv_set_snapshots(eng.h, None), "spectrum": lambda: lib.wv_set_spectrum(eng.h, None, None),
          "decay": lambda: lib.wv_set_decay(eng.h, None), "decay_bands": lambda: lib.wv_set_decay_bands(eng.h, None, None, 0, 0),
          "intensity": lambda: lib.wv_set_intensity(eng.h, None), "arrival": lambda: lib.wv_set_arrival(eng.h, None, None),
          "lateral": lambda: lib.wv_set_lateral(eng.h, None, None), "modulation": lambda: lib.wv_set_modulation(eng.h, None, None, None, 0, 0)}[kind]()
    assert rc == 0, (kind, rc)


def answer(eng, kind, faults):
    """[code, sentence] of the setter's refusal of the valid plan with `faults` applied in order; None where the plan was taken (it is
    stopped again)."""
    args = dict(BASE[kind])
    for name in faults:
        FAULTS[kind][name](args)
    rc = call(eng, kind, args)
    if rc == 0:
        stop(eng, kind)
        return None
    return [rc, eng.lib.wv_last_error().decode()]


def make_engine():
    """The engine of every case: fp32, both fields filled, three steps taken."""
    from wayverb_amd import engine as E
    from wayverb_amd import mesh as M
    eng = E.Engine(M.box_mesh(*MESH), precision="f32")
    rng = np.random.default_rng(18)
    for buffer in (E.BUF_CURRENT, E.BUF_PREVIOUS):
        eng.write_field((rng.standard_normal(MESH[0] * MESH[1] * MESH[2]) * 1e-3).astype(np.float32), buffer)
    for _ in range(3):
        eng.step()
    return eng


def state(eng):
    from wayverb_amd import engine as E
    return eng.step_count(), eng.read_field(E.BUF_CURRENT).tobytes(), eng.read_field(E.BUF_PREVIOUS).tobytes()


def observe(eng, kind, check=lambda: None):
    """dict(answers, single, pairs) of one setter: `check` is called after every case."""
    names = list(FAULTS[kind])
    answers = []

    def index(faults):
        got = answer(eng, kind, faults)
        check()
        if got is None:
            return None
        if got not in answers:
            answers.append(got)
        return answers.index(got)

    single = {name: index([name]) for name in names}
    pairs = {first: [index([first, second]) for second in names] for first in names}
    return dict(faults=names, answers=answers, single=single, pairs=pairs)


def observe_split(eng):
    """The one STATE refusal that is a setter's own: under an active plain decay plan the banded setter says so, whatever else is wrong
    with its arguments; under a banded plan the plain setter answers in the words every plan's setter has."""
    out = {}
    for active, setter in (("decay", "decay_bands"), ("decay_bands", "decay")):
        assert call(eng, active, dict(BASE[active])) == 0
        out[setter] = {"valid": answer(eng, setter, [])}
        out[setter].update({name: answer(eng, setter, [name]) for name in FAULTS[setter]})
        stop(eng, active)
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/plan_argument_faults.py --record    (on a GPU; rewrites tests/golden/plan_argument_refusals.json)")
    engine = make_engine()
    recorded = {kind: observe(engine, kind) for kind in KINDS}
    recorded["decay split"] = observe_split(engine)
    engine.close()
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("recorded", GOLDEN, os.path.getsize(GOLDEN), "bytes")
