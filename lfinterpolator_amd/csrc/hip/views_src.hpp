// views_src.hpp — where a kernel that READS rendered views finds them: the one description behind the quilt, the scaled quilt, the YUV
// frames and the native image (the host side fills it in: rendered_views, lfi_context.hpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace lfi {

// RGBA planes [view][H][W] (pitch == 0), or byte planes [view][R,G,B][H][pitch] (the planar layout, blend_p3.hpp).  Not only the context's
// views: a quilt one tile wide, or a whole quilt taken as ONE view, is described the same way.
struct ViewsSrc
{
    const uint8_t *base;  // view 0: the call's first view, or the context's where the kernel's arguments hold a v0 of their own
    size_t view_stride;   // bytes from view to view
    uint32_t W, H;        // the size of a view (under a row window H is the band's rows: the rows the views hold)
    uint32_t pitch;       // bytes per row of a byte plane, a multiple of 128; 0: the views are RGBA
};

} // namespace lfi
