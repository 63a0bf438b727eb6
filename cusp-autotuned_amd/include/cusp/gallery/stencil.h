// cusp/gallery/stencil.h -- cusp::gallery::generate_matrix_from_stencil (reference cusp/gallery/stencil.h).
// The generator lives with the Poisson stencils in poisson.h; this header exists so that the reference's include line works.
#pragma once
#include "poisson.h"
