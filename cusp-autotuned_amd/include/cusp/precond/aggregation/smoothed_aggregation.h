// cusp/precond/aggregation/smoothed_aggregation.h -- smoothed_aggregation<IndexType, ValueType, MemorySpace>: algebraic
// multigrid by smoothed aggregation, usable as the preconditioner M of every cusp::krylov solver that takes one
// (reference cusp/precond/aggregation/smoothed_aggregation.h, detail/smoothed_aggregation.inl).
//   smoothed_aggregation<int, double, cusp::device_memory> M(A);  cusp::krylov::cg(A, x, b, monitor, M);
// A: any of the five formats, converted to CSR for set-up.  Per level: strength (theta) -> standard_aggregate (host; with
// mis_aggregation set: mis_aggregate, which on device_memory makes no host copy of the structure) -> fit_candidates ->
// smooth_prolongator -> form_restriction -> galerkin_product, until a level has at most min_level_size rows (500) or
// max_levels (10) exist; Jacobi smoothing; a dense LU on the coarsest level.  Each device_memory component returns the
// bits of this project's host_memory path, which is the reference's sequential algorithm.
// (The device sparse product alone keeps exact-zero sums that the host product drops; galerkin_product removes them, see there.
// The rho estimate is the one number the two spaces may round differently: sa_level::rho_DinvA records what each used.)
// Deviation: rho(D^-1 A) is estimated ONCE per level, kept in sa_level::rho_DinvA and used for the prolongator and the
// smoother (the reference passes it by value and so estimates it twice).
// mis_aggregation (public, false by default): set it on a default-constructed object before initialize(A) to aggregate every
// level with mis_aggregate instead of standard_aggregate; the cross-space constructor copies it.
// evolution_strength (public, false by default) with evolution_epsilon (4): set them the same way to take every level's strength
// matrix from evolution_strength_of_connection(A, C, B, rho_DinvA, evolution_epsilon) instead of the symmetric measure; the
// level's rho is then estimated before the strength step (still once per level) and theta is not used.  Combines with
// mis_aggregation.  With the flag clear the order of calls and every bit are what they were.
// Not built: other smoothers, several candidate vectors, a sharded hierarchy.
#pragma once
#include "../../detail/multilevel.h"
#include "../smoother/jacobi_smoother.h"
#include "aggregate.h"
#include "galerkin_product.h"
#include "restrict.h"
#include "smooth_prolongator.h"
#include "strength.h"
#include "tentative.h"

namespace cusp {
namespace precond {
namespace aggregation {

template <typename IndexType, typename ValueType, typename MemorySpace> struct sa_level {
    cusp::csr_matrix<IndexType, ValueType, MemorySpace> A_;  // this level's operator (set-up copy)
    cusp::array1d<IndexType, MemorySpace> aggregates;
    cusp::array1d<ValueType, MemorySpace> B;                 // the candidate vector
    double rho_DinvA = 0.0;
    sa_level() {}
    template <typename L2> sa_level(const L2 &o) : A_(o.A_), aggregates(o.aggregates), B(o.B), rho_DinvA(o.rho_DinvA) {}
};

template <typename IndexType, typename ValueType, typename MemorySpace>
class smoothed_aggregation
    : public cusp::multilevel<cusp::csr_matrix<IndexType, ValueType, MemorySpace>, cusp::precond::jacobi_smoother<ValueType, MemorySpace>, cusp::detail::lu_solver<ValueType, MemorySpace>> {
    typedef cusp::csr_matrix<IndexType, ValueType, MemorySpace> Csr;
    typedef cusp::multilevel<Csr, cusp::precond::jacobi_smoother<ValueType, MemorySpace>, cusp::detail::lu_solver<ValueType, MemorySpace>> Parent;

public:
    double theta = 0.0;
    bool mis_aggregation = false; // aggregate with mis_aggregate (MIS(2)) instead of standard_aggregate; read by extend_hierarchy
    bool evolution_strength = false; // strength from evolution_strength_of_connection instead of the symmetric measure; read by extend_hierarchy
    double evolution_epsilon = 4.0;  // its distance filter
    std::vector<sa_level<IndexType, ValueType, MemorySpace>> sa_levels;

    smoothed_aggregation() {}
    template <typename MatrixType> smoothed_aggregation(const MatrixType &A, double theta_ = 0.0, size_t min_level_size_ = 500, size_t max_levels_ = 10) : theta(theta_)
    {
        this->min_level_size = min_level_size_;
        this->max_levels = max_levels_;
        initialize(A);
    }
    template <typename MatrixType, typename ArrayType>
    smoothed_aggregation(const MatrixType &A, const ArrayType &B, double theta_ = 0.0, size_t min_level_size_ = 500, size_t max_levels_ = 10,
                         typename std::enable_if<!std::is_arithmetic<ArrayType>::value>::type * = nullptr)
        : theta(theta_)
    {
        this->min_level_size = min_level_size_;
        this->max_levels = max_levels_;
        initialize(A, B);
    }
    template <typename MemorySpace2>
    smoothed_aggregation(const smoothed_aggregation<IndexType, ValueType, MemorySpace2> &o) : Parent(o), theta(o.theta), mis_aggregation(o.mis_aggregation), evolution_strength(o.evolution_strength), evolution_epsilon(o.evolution_epsilon)
    {
        for (size_t i = 0; i < o.sa_levels.size(); i++) sa_levels.push_back(sa_level<IndexType, ValueType, MemorySpace>(o.sa_levels[i]));
    }

    template <typename MatrixType> void initialize(const MatrixType &A)
    {
        cusp::array1d<ValueType, MemorySpace> B(A.num_rows, ValueType(1));
        initialize(A, B);
    }
    template <typename MatrixType, typename ArrayType> void initialize(const MatrixType &A, const ArrayType &B)
    {
        if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("smoothed_aggregation: matrix must be square");
        if (B.size() != A.num_rows) throw cusp::invalid_input_exception("smoothed_aggregation: the candidate vector must have the matrix's size");
        this->levels.clear();
        sa_levels.clear();
        sa_levels.emplace_back();
        sa_levels.back().A_ = A; // (any format: converted to CSR in MemorySpace)
        sa_levels.back().B = B;
        while (sa_levels.back().A_.num_rows > this->min_level_size && sa_levels.size() < this->max_levels) extend_hierarchy();
        this->levels.emplace_back();
        this->levels.back().A = sa_levels.back().A_;
        this->initialize_coarse_solver();
    }

private:
    void extend_hierarchy()
    {
        sa_level<IndexType, ValueType, MemorySpace> &cur = sa_levels.back();
        const Csr &A = cur.A_;
        Csr C, T, P, R, RAP;
        cusp::array1d<ValueType, MemorySpace> B_coarse;
        if (evolution_strength) {
            cur.rho_DinvA = cusp::eigen::estimate_rho_Dinv_A(A);
            evolution_strength_of_connection(A, C, cur.B, cur.rho_DinvA, evolution_epsilon);
        } else symmetric_strength_of_connection(A, C, theta);
        if (mis_aggregation) mis_aggregate(C, cur.aggregates);
        else standard_aggregate(C, cur.aggregates);
        fit_candidates(cur.aggregates, cur.B, T, B_coarse);
        if (!evolution_strength) cur.rho_DinvA = cusp::eigen::estimate_rho_Dinv_A(A);
        smooth_prolongator(A, T, P, cur.rho_DinvA);
        form_restriction(P, R);
        galerkin_product(R, A, P, RAP);

        this->levels.emplace_back();
        typename Parent::level &L = this->levels.back();
        L.A = A;
        L.smoother = cusp::precond::jacobi_smoother<ValueType, MemorySpace>(A, cur.rho_DinvA);
        L.R.swap(R);
        L.P.swap(P);
        sa_levels.emplace_back(); // (cur is dangling from here)
        sa_levels.back().A_.swap(RAP);
        sa_levels.back().B = B_coarse;
    }
};

} // namespace aggregation
} // namespace precond
} // namespace cusp
