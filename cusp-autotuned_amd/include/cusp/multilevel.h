// cusp/multilevel.h -- the reference's include path of cusp::multilevel (the class lives in cusp/detail/multilevel.h).
#pragma once
#include "detail/multilevel.h"
