// adsb_fmt.cpp -- the host side of the sample formats a decimator or a resampler takes beside CS16 and 8-bit
// (include/adsb_hip.h, "Sample formats"): the CF32 scale's check and its setters.  The scale is host state that every
// launch carries in its parameters, so nothing here touches the device or the stream; the conversion itself is
// adsb_fmt_dev.h's.  The handles are adsb_decim.cpp's, adsb_resamp.cpp's and adsb_bank.cpp's: scale_of reaches into them (the two getters
// live beside the handles, as the mixer's do).
#include <cmath>

#include "adsb_ctx.h"

using namespace adsb::host;

namespace {

// finite, 0 < g <= 2^31 (a NaN fails the first comparison)
int scale_set(float *slot, float scale)
{
    if (!(scale > 0.0f) || !(scale <= kInMaxScale) || !std::isfinite(scale)) return ADSB_ERR_INVALID;
    *slot = scale;
    return ADSB_OK;
}

}  // namespace

extern "C" {

int adsb_fmt_set_scale_decim(adsb_decim *d, float scale) { return d ? scale_set(scale_of(d), scale) : ADSB_ERR_INVALID; }

int adsb_fmt_set_scale_resamp(adsb_resamp *r, float scale) { return r ? scale_set(scale_of(r), scale) : ADSB_ERR_INVALID; }

int adsb_bank_set_scale(adsb_bank *b, float scale) { return b ? scale_set(scale_of(b), scale) : ADSB_ERR_INVALID; }

}  // extern "C"
