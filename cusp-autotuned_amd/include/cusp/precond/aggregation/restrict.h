// cusp/precond/aggregation/restrict.h -- form_restriction(P, R): R = P^T through cusp::transpose
// (reference cusp/precond/aggregation/restrict.h); the stable sort keeps a column's entries in row order in both spaces.
#pragma once
#include "../../transpose.h"

namespace cusp {
namespace precond {
namespace aggregation {

template <typename MatrixType1, typename MatrixType2> void form_restriction(const MatrixType1 &P, MatrixType2 &R) { cusp::transpose(P, R); }

} // namespace aggregation
} // namespace precond
} // namespace cusp
