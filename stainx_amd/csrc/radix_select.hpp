// The bookkeeping of the exact three-pass radix selection over order-preserving float keys (common.hpp: float_key): 11 / 11 / 10 key
// bits per pass, one integer histogram per pass, and the state a one-workgroup step leaves for the next pass.  Shared by the
// percentile concentrations (vahadane.hpp) and the luminosity percentile (luminosity.hpp).
#pragma once

#include "common.hpp"

namespace sx {
namespace radix {

constexpr int kBits0 = 11, kBits1 = 11, kBits2 = 10;
constexpr int kBinsAll = (1 << kBits0) + (1 << kBits1) + (1 << kBits2);      // 5120 counts per selection

struct SelectState {      // per selection
    unsigned long long rank;      // the wanted rank (1-based) among the keys that share `prefix`
    unsigned long long count;     // |S|
    uint32_t prefix;              // the key's leading bits found so far
    uint32_t pad;
};

template <int kPass> struct PassBins {
    static constexpr int bits = kPass == 0 ? kBits0 : (kPass == 1 ? kBits1 : kBits2);
    static constexpr int offset = kPass == 0 ? 0 : (kPass == 1 ? (1 << kBits0) : (1 << kBits0) + (1 << kBits1));
    static constexpr int below = kPass == 0 ? kBits1 + kBits2 : (kPass == 1 ? kBits2 : 0);      // key bits below this pass's digit
};

}  // namespace radix
}  // namespace sx
