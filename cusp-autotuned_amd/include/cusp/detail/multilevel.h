// cusp/detail/multilevel.h -- cusp::multilevel<MatrixType, SmootherType, SolverType>: the levels of a multigrid hierarchy and its
// cycle (reference cusp/multilevel.h, detail/multilevel.inl), restated step by step:
//   operator()(b, x) : one V-cycle from x = 0.  Per level: presmooth; residual = b - A x (cusp::multiply, then axpby);
//                      coarse b = R residual; recurse; x += P (coarse x); postsmooth.  Coarsest level: the LU solve -- its right-hand
//                      side goes to the host, through lu_solver, and back.
//   solve(b, x[, monitor]) : x += cycle(residual) until the monitor is satisfied.
// On device_memory every multiply goes through the containers' plans; the vectors stay in HBM except on the coarsest level.
// The members the cycle writes are mutable: a preconditioner is applied through a const reference by cusp::krylov.
#pragma once
#include <cstdio>
#include <vector>

#include "../blas/blas.h"
#include "../linear_operator.h"
#include "../monitor.h"
#include "../multiply.h"
#include "lu.h"

namespace cusp {

template <typename MatrixType, typename SmootherType, typename SolverType>
class multilevel : public cusp::linear_operator<typename MatrixType::value_type, typename MatrixType::memory_space> {
public:
    typedef typename MatrixType::index_type IndexType;
    typedef typename MatrixType::value_type ValueType;
    typedef typename MatrixType::memory_space MemorySpace;

    struct level {
        MatrixType R, A, P; // restriction, operator, prolongation (R and P empty on the coarsest level)
        mutable cusp::array1d<ValueType, MemorySpace> x, b, residual;
        mutable SmootherType smoother;
        level() {}
        template <typename Level2> level(const Level2 &o) : R(o.R), A(o.A), P(o.P), x(o.x), b(o.b), residual(o.residual), smoother(o.smoother) {}
    };

    size_t min_level_size = 500, max_levels = 10;
    std::vector<level> levels;
    SolverType solver;

    multilevel() {}
    template <typename M2, typename S2, typename V2> multilevel(const multilevel<M2, S2, V2> &o) : min_level_size(o.min_level_size), max_levels(o.max_levels), solver(o.solver)
    {
        this->num_rows = o.num_rows; this->num_cols = o.num_cols; this->num_entries = o.num_entries;
        for (size_t i = 0; i < o.levels.size(); i++) levels.push_back(level(o.levels[i]));
    }

    void set_min_level_size(size_t n) { min_level_size = n; }
    void set_max_levels(size_t n) { max_levels = n; }

    // call once the levels are in place: sizes the work vectors and factors the coarsest operator
    void initialize_coarse_solver()
    {
        for (size_t i = 0; i < levels.size(); i++) {
            levels[i].x.resize(levels[i].A.num_rows);
            levels[i].b.resize(levels[i].A.num_rows);
            levels[i].residual.resize(levels[i].A.num_rows);
        }
        solver = SolverType(levels.back().A);
        this->num_rows = this->num_cols = levels[0].A.num_rows;
        this->num_entries = levels[0].A.num_entries;
    }

    template <typename Array1, typename Array2> void operator()(const Array1 &b, Array2 &x) const { cycle(b, x, 0); }

    template <typename Array1, typename Array2> void solve(const Array1 &b, Array2 &x) const
    {
        cusp::monitor<ValueType> monitor(b);
        solve(b, x, monitor);
    }
    template <typename Array1, typename Array2, typename Monitor> void solve(const Array1 &b, Array2 &x, Monitor &monitor) const
    {
        const MatrixType &A = levels[0].A;
        cusp::array1d<ValueType, MemorySpace> update(A.num_rows), residual(A.num_rows);
        cusp::multiply(A, x, residual);
        cusp::blas::axpby(b, residual, residual, ValueType(1), ValueType(-1));
        while (!monitor.finished(residual)) {
            cycle(residual, update, 0);
            cusp::blas::axpy(update, x, ValueType(1));
            cusp::multiply(A, x, residual);
            cusp::blas::axpby(b, residual, residual, ValueType(1), ValueType(-1));
            ++monitor;
        }
    }

    double operator_complexity() const
    {
        size_t n = 0;
        for (size_t i = 0; i < levels.size(); i++) n += levels[i].A.num_entries;
        return double(n) / double(levels[0].A.num_entries);
    }
    double grid_complexity() const
    {
        size_t n = 0;
        for (size_t i = 0; i < levels.size(); i++) n += levels[i].A.num_rows;
        return double(n) / double(levels[0].A.num_rows);
    }
    void print() const
    {
        std::printf("\tNumber of Levels:\t%zu\n\tOperator Complexity:\t%f\n\tGrid Complexity:\t%f\n\tlevel\tunknowns\tnonzeros\n", levels.size(), operator_complexity(), grid_complexity());
        for (size_t i = 0; i < levels.size(); i++) std::printf("\t%zu\t%zu\t\t%zu\n", i, levels[i].A.num_rows, levels[i].A.num_entries);
    }

private:
    template <typename Array1, typename Array2> void cycle(const Array1 &b, Array2 &x, size_t i) const
    {
        if (i + 1 == levels.size()) {
            solver(b, x);
            return;
        }
        const level &L = levels[i];
        L.smoother.presmooth(L.A, b, x);
        cusp::multiply(L.A, x, L.residual);
        cusp::blas::axpby(b, L.residual, L.residual, ValueType(1), ValueType(-1));
        cusp::multiply(L.R, L.residual, levels[i + 1].b);
        cycle(levels[i + 1].b, levels[i + 1].x, i + 1);
        cusp::multiply(L.P, levels[i + 1].x, L.residual);
        cusp::blas::axpy(L.residual, x, ValueType(1));
        L.smoother.postsmooth(L.A, b, x);
    }
};

} // namespace cusp
