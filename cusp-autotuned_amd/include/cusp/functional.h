// cusp/functional.h -- the functors the 7-argument cusp::multiply is called with
// (reference cusp/functional.h; generic/multiply.inl:104-110 uses constant_functor(0), multiplies, plus).
// minimum, maximum, project1st and project2nd are spelled as thrust spells them: ties and NaNs follow the definitions below, not fmin / fmax
// (minimum(1, NaN) is NaN and minimum(NaN, 1) is 1, so minimum(minimum(1, NaN), 2) = 2 while minimum(1, minimum(NaN, 2)) = 1: a chain of
// them depends on its order).  combine is called as combine(matrix value, vector value).
#pragma once
namespace cusp {
template <typename T> struct plus { T operator()(const T &a, const T &b) const { return a + b; } };
template <typename T> struct multiplies { T operator()(const T &a, const T &b) const { return a * b; } };
template <typename T> struct minimum { T operator()(const T &a, const T &b) const { return a < b ? a : b; } };
template <typename T> struct maximum { T operator()(const T &a, const T &b) const { return a < b ? b : a; } };
template <typename T> struct project1st { T operator()(const T &a, const T &) const { return a; } };
template <typename T> struct project2nd { T operator()(const T &, const T &b) const { return b; } };
template <typename T> struct identity_function { T operator()(const T &a) const { return a; } };
template <typename T> struct constant_functor {
    T value;
    explicit constant_functor(T v = T(0)) : value(v) {}
    T operator()(const T &) const { return value; }
};
} // namespace cusp
