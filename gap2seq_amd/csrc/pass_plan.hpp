// gap2seq_amd/csrc/pass_plan.hpp — the key-range passes of the solid k-mer count (solid_passes.h), planned on the host.
//
// A histogram of the keys over consecutive, equally wide key ranges (bins) is cut, in key order, into passes: runs of
// consecutive bins that hold at most `cap` keys together.  The cut is greedy: a pass is closed in front of the first bin
// that would take it beyond cap.  A bin that alone holds more than cap keys therefore stands alone in its pass (the bin
// after it, even an empty one, opens the next pass); the caller histograms such a bin again on finer bins.  Empty bins
// join the pass that is open, so the bins in front of an oversized bin may form a pass without keys.
// Plain host code: no HIP, no device.
#pragma once
#include <cstdint>
#include <vector>

namespace g2s {

// first_bin[p] = the first bin of pass p, first_bin[passes] = nbins; every pass has at least one bin.  Returns the number
// of passes (0 for nbins == 0).  *first_oversized = the first bin with more than cap keys, or nbins when there is none.
uint32_t plan_passes(const uint64_t* hist, uint32_t nbins, uint64_t cap, std::vector<uint32_t>* first_bin,
                     uint32_t* first_oversized);

}  // namespace g2s
