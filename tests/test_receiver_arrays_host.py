"""CPU: wv_directional_accumulate (csrc/postprocess.cpp), the host twin of the kernel behind wv_set_directional_receivers, against
postprocess.directional_receiver -- the Python restatement of postprocessor::directional_receiver that every GPU test of the
receivers uses as its yardstick.  Bitwise, on seeded random traces; spacing and density as simulation.canonical has them."""
import numpy as np
import pytest

from helpers import canonical_parameters
from wayverb_amd import postprocess as P
from wayverb_amd import simulation as W

STEPS = 500



def traces(valued, seed):
    """Columns as an fp32 / fp64 engine delivers them (doubles either way; an fp32 engine's are float-valued): a common part that
    all seven share plus small differences, as neighbouring nodes of a field have them, over several orders of magnitude."""
    rng = np.random.default_rng(seed)
    common = rng.uniform(-1.0, 1.0, (STEPS, 1)) * 10.0 ** rng.uniform(-6, 0, (STEPS, 1))
    p7 = common + rng.uniform(-1.0, 1.0, (STEPS, 7)) * 10.0 ** rng.uniform(-9, -1, (STEPS, 7))
    p7[3] = 0.0                                    # a silent step
    p7[4, 1:] = p7[4, 0]                           # no gradient
    return p7.astype(valued).astype(np.float64)


@pytest.mark.parametrize("valued", [np.float32, np.float64], ids=["fp32-valued", "fp64-valued"])
@pytest.mark.parametrize("seed", [1, 2])
def test_library_integrator_equals_the_python_yardstick(built_library, valued, seed):
    spacing, sample_rate, density = canonical_parameters()
    p7 = traces(valued, seed)
    want = P.directional_receiver(p7, spacing, sample_rate, density)
    velocity = np.zeros(3)
    got = P.directional_accumulate(p7, spacing, sample_rate, density, velocity)
    assert got.dtype == P.directional_output_dtype and got.shape == (STEPS,)
    assert got.tobytes() == want.tobytes()
    assert np.abs(got["intensity"]).max() > 0 and np.abs(velocity).max() > 0
    assert got["pressure"].tobytes() == p7[:, 0].astype(np.float32).tobytes()


@pytest.mark.parametrize("valued", [np.float32, np.float64], ids=["fp32-valued", "fp64-valued"])
def test_one_call_equals_three_calls_that_carry_the_velocity(built_library, valued):
    spacing, sample_rate, density = canonical_parameters()
    p7 = traces(valued, 3)
    v_one = np.zeros(3)
    one = P.directional_accumulate(p7, spacing, sample_rate, density, v_one)
    v = np.zeros(3)
    parts = [P.directional_accumulate(p7[a:b], spacing, sample_rate, density, v) for a, b in ((0, 1), (1, 190), (190, STEPS))]
    assert np.concatenate(parts).tobytes() == one.tobytes()
    assert v.tobytes() == v_one.tobytes()
    # (no velocity handed in: from rest)
    assert P.directional_accumulate(p7, spacing, sample_rate, density).tobytes() == one.tobytes()


def test_bad_arguments_are_refused(built_library):
    from wayverb_amd import engine as E
    p7 = np.zeros((4, 7))
    for spacing, rate, density in ((0.0, 1000.0, 1.2), (0.4, 0.0, 1.2), (0.4, 1000.0, -1.0)):
        with pytest.raises(E.WaveguideError, match="error -1"):
            P.directional_accumulate(p7, spacing, rate, density)
    assert P.directional_accumulate(np.zeros((0, 7)), 0.4, 1000.0, 1.2).shape == (0,)
