// cusp/eigen/lanczos_options.h -- the options of cusp::eigen::lanczos (reference cusp/eigen/lanczos_options.h: the same enums, field names and
// defaults).  minIter, maxIter == 0, stride == 0, memoryExpansionFactor <= 1 and tol < 0 mean "choose for me"; lanczos() writes what it chose
// back into the object, as the reference does.
#pragma once
#include <cmath>
#include <cstddef>
#include <iostream>
#include <limits>

namespace cusp {
namespace eigen {

typedef enum { SA, LA, BE } SpectrumPart;   // smallest algebraic, largest algebraic, both ends (the low end takes wanted / 2)
typedef enum { None, Full } ReorthStrategy; // Full: every new vector against ALL stored ones (lanczos.h, departure b)

template <typename ValueType> class lanczos_options {
public:
    bool computeEigVecs;
    bool verbose;

    size_t minIter;   // the first convergence check is made at this many steps
    size_t maxIter;
    size_t extraIter; // steps between the first passed check and the confirming one
    size_t stride;    // steps between checks

    ReorthStrategy reorth;
    SpectrumPart eigPart;

    ValueType memoryExpansionFactor;
    ValueType tol; // on the relative change of the sum of the wanted Ritz values between two consecutive steps
    ValueType doubleReorthGamma;
    ValueType localReorthGamma;

    size_t defaultMinIterFactor;
    size_t defaultMaxIterFactor;

    ValueType eigLowCut;  // only Ritz values <= eigLowCut count at the low end
    ValueType eigHighCut; // only Ritz values >= eigHighCut count at the high end

    lanczos_options()
        : computeEigVecs(false), verbose(false), minIter(0), maxIter(0), extraIter(10), stride(10), reorth(None), eigPart(LA), memoryExpansionFactor(1.2),
          tol(1e-4), doubleReorthGamma(1.0 / std::sqrt(2.0)), localReorthGamma(1.0 / std::sqrt(2.0)), defaultMinIterFactor(5), defaultMaxIterFactor(50),
          eigLowCut(std::numeric_limits<ValueType>::infinity()), eigHighCut(-std::numeric_limits<ValueType>::infinity())
    {}
    lanczos_options(const lanczos_options &) = default;

    void print() const
    {
        static const char *const parts[] = {"SA", "LA", "BE"};
        static const char *const strategies[] = {"None", "Full"};
        std::cout << "lanczos_options:"
                  << "\n  computeEigVecs        " << computeEigVecs << "\n  verbose               " << verbose << "\n  minIter               " << minIter
                  << "\n  maxIter               " << maxIter << "\n  extraIter             " << extraIter << "\n  stride                " << stride
                  << "\n  reorth                " << strategies[reorth] << "\n  eigPart               " << parts[eigPart] << "\n  memoryExpansionFactor "
                  << memoryExpansionFactor << "\n  tol                   " << tol << "\n  doubleReorthGamma     " << doubleReorthGamma
                  << "\n  localReorthGamma      " << localReorthGamma << "\n  defaultMinIterFactor  " << defaultMinIterFactor << "\n  defaultMaxIterFactor  "
                  << defaultMaxIterFactor << "\n  eigLowCut             " << eigLowCut << "\n  eigHighCut            " << eigHighCut << std::endl;
    }
};

} // namespace eigen
} // namespace cusp
