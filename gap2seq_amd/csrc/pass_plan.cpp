// gap2seq_amd/csrc/pass_plan.cpp — see pass_plan.hpp.
#include "pass_plan.hpp"

namespace g2s {

uint32_t plan_passes(const uint64_t* hist, uint32_t nbins, uint64_t cap, std::vector<uint32_t>* first_bin,
                     uint32_t* first_oversized) {
  first_bin->clear();
  uint32_t over = nbins;
  uint64_t sum = 0;  // the keys of the open pass, bins [first_bin->back(), b)
  for (uint32_t b = 0; b < nbins; b++) {
    const uint64_t h = hist[b];
    if (h > cap && over == nbins) over = b;
    // (sum <= cap, or the open pass is one oversized bin: either way no wrap-around in the comparison)
    const bool fits = sum <= cap && h <= cap - sum;
    if (b == 0 || !fits) { first_bin->push_back(b); sum = 0; }
    sum += h;
  }
  const uint32_t passes = (uint32_t)first_bin->size();
  first_bin->push_back(nbins);
  if (first_oversized) *first_oversized = over;
  return passes;
}

}  // namespace g2s
