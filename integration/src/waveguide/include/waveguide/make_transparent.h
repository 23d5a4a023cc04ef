// Forwarding header in place of src/waveguide/include/waveguide/make_transparent.h (reference: make_transparent.cpp:10-30):
// `waveguide::make_transparent(begin, end)` keeps its signature, its mesh impulse response is made on the MI355X at first use
// instead of being compiled in (mesh_impulse_response.h is no longer generated).  bin/boundary_test, bin/solution_growth and
// the reference's waveguide tests call it as before; `compressed_rectangular_waveguide` comes with it.
#pragma once

#include "waveguide/waveguide.h"

#include "wayverb_amd/compensation_signal.h"
