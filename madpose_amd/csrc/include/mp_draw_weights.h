// The quantisation of the confidence weights of mp_draw_weights_create: the one place where
// the weighted draw touches floating point (include/mp_draw.h, the sampler, stays integer-only).
// One function for host and device.
//
// A weight is a float32 (converted to double first, which is exact) or a float64.  Valid weights
// are finite and lie in 0 <= w <= 1; q = min(65535, floor(w * 65536)) as uint32.  The product is
// with a power of two and therefore exact (a subnormal result can only round below 1, where the
// floor is 0 either way); there is no division and no expression a fused multiply-add could
// change.  q = 0 masks the correspondence.
#pragma once
#include "mp_draw.h"

namespace mp {

// q of one weight; false (and q = 0) for a NaN, an infinity, a negative value or a value above 1
MP_HD bool draw_quantise(double w, uint32_t *q) {
    *q = 0;
    if (!(w >= 0.0) || !(w <= 1.0)) return false;
    const uint32_t v = (uint32_t)(w * 65536.0); // (0 .. 65536; the conversion truncates: the floor)
    *q = v > kDrawWeightQMax ? kDrawWeightQMax : v;
    return true;
}

} // namespace mp
