// STAND-IN for <ocs2_core/control/LinearController.h> (+ the matrix_t of <ocs2_core/Types.h> and LinearInterpolation::timeSegment of
// <ocs2_core/misc/LinearInterpolation.h>): the time-varying affine policy u(t, x) = uff(t) + K(t) x.  Upstream declares matrix_t (an
// Eigen::MatrixXd) in Types.h; this minimal stand-in lives here so that the existing Types.h stand-in stays as it is.
#pragma once
#include <algorithm>
#include <utility>

#include <ocs2_core/control/FeedforwardController.h>
namespace ocs2 {
class matrix_t {   // the subset of Eigen::MatrixXd the adaptor uses: element access (i, j), rows(), cols()
 public:
  matrix_t() = default;
  matrix_t(size_t rows, size_t cols) : r_(rows), c_(cols), v_(rows * cols, 0.0) {}
  scalar_t& operator()(size_t i, size_t j) { return v_[j * r_ + i]; }   // column-major like Eigen's default
  const scalar_t& operator()(size_t i, size_t j) const { return v_[j * r_ + i]; }
  size_t rows() const { return r_; }
  size_t cols() const { return c_; }
 private:
  size_t r_ = 0, c_ = 0;
  std::vector<scalar_t> v_;
};
using matrix_array_t = std::vector<matrix_t>;

namespace LinearInterpolation {
// {index, alpha}: the value at t is alpha * v[index] + (1 - alpha) * v[index + 1]; lookup::findIndexInTimeArray is std::lower_bound
inline std::pair<int, scalar_t> timeSegment(scalar_t t, const scalar_array_t& times) {
  if (times.size() <= 1) return {0, 1.0};
  const int index = (int)(std::lower_bound(times.begin(), times.end(), t) - times.begin());
  const int last = (int)times.size() - 1;
  if (index <= 0) return {0, 1.0};
  if (index > last) return {last - 1, 0.0};
  return {index - 1, (times[index] - t) / (times[index] - times[index - 1])};
}
}  // namespace LinearInterpolation

class LinearController final : public ControllerBase {
 public:
  LinearController(scalar_array_t times, vector_array_t bias, matrix_array_t gain)
      : timeStamp_(std::move(times)), biasArray_(std::move(bias)), gainArray_(std::move(gain)) {}
  vector_t computeInput(scalar_t t, const vector_t& x) override {
    const std::pair<int, scalar_t> ia = LinearInterpolation::timeSegment(t, timeStamp_);
    const size_t i0 = ia.first, i1 = std::min<size_t>(ia.first + 1, timeStamp_.size() - 1);
    const scalar_t a = ia.second;
    const matrix_t& K0 = gainArray_[i0];
    const matrix_t& K1 = gainArray_[i1];
    vector_t u(biasArray_[i0].size());
    for (size_t r = 0; r < u.size(); ++r) {
      scalar_t kx = 0.0;
      for (size_t c = 0; c < K0.cols(); ++c) kx += (a * K0(r, c) + (1.0 - a) * K1(r, c)) * x[c];
      u[r] = (a * biasArray_[i0][r] + (1.0 - a) * biasArray_[i1][r]) + kx;
    }
    return u;
  }
  scalar_array_t timeStamp_;
  vector_array_t biasArray_;
  matrix_array_t gainArray_;
};
}  // namespace ocs2
