// Keeping the source's blocks (mdhip_jpeg_encode_kept, mdjpeg_keep_merge): which MCUs of a window a list of changed
// rectangles touches, and where the blocks of an MCU lie in the source's coefficient planes.  ONE predicate and ONE
// addressing rule, compiled by the coefficient kernel (jpeg_encode.cpp) and by the host model (jpeg_encode_host.cpp), the
// arrangement of jpeg_encode.h, blur_box.h and resample.h.
//
// A rectangle is left, top, right, bottom in pixels of its window, right and bottom exclusive (mdhip_blur_regions'
// convention).  It is clipped to the window first, and one without area after that is dropped: an edge MCU reaches beyond
// the window, so an unclipped rectangle beside the window would otherwise touch it.  MCU (mx, my) of a window with luma
// sampling (hs, vs) covers the pixels [mx * 8hs, (mx + 1) * 8hs) x [my * 8vs, (my + 1) * 8vs) and is CHANGED iff some
// rectangle of the window has left < (mx + 1) * 8hs, right > mx * 8hs, top < (my + 1) * 8vs and bottom > my * 8vs.
//
// The source's planes are in the layout of mdjpeg_decode for three components and whole MCUs: Y [mcus_y * vs][mcus_x * hs][64],
// then Cb and Cr [mcus_y][mcus_x][64] each, natural order within a block.
#ifndef MDJPEG_KEEP_H
#define MDJPEG_KEEP_H

#include <stdint.h>

#include "jpeg_encode.h"

struct MdjKeepRect {
    int32_t left, top, right, bottom;
};

// clips q[0 .. 3] to a width x height window; false: nothing of it is left
MDJ_HD bool mdj_keep_clip(const int32_t* q, int width, int height, MdjKeepRect* out) {
    out->left = q[0] > 0 ? q[0] : 0;
    out->top = q[1] > 0 ? q[1] : 0;
    out->right = q[2] < width ? q[2] : width;
    out->bottom = q[3] < height ? q[3] : height;
    return out->right > out->left && out->bottom > out->top;
}

// MCU (mx, my) is touched by one of the clipped rectangles rects[lo .. hi)
MDJ_HD bool mdj_keep_changed(const MdjKeepRect* rects, int lo, int hi, int mx, int my, int hs, int vs) {
    const int x0 = mx * 8 * hs, x1 = x0 + 8 * hs, y0 = my * 8 * vs, y1 = y0 + 8 * vs;
    for (int i = lo; i < hi; ++i) {
        const MdjKeepRect q = rects[i];
        if (q.left < x1 && q.right > x0 && q.top < y1 && q.bottom > y0) return true;
    }
    return false;
}

// int16 values of the source planes of a crop: what the caller's blocks_w / blocks_h have to describe
MDJ_HD int64_t mdj_keep_plane_values(const MdjEncCrop& c) { return int64_t(c.mcus_x) * c.mcus_y * c.per_mcu * 64; }

// first value of block k of MCU (mx, my) in the source planes (block k as in jpeg_encode.h: luma (k % hs, k / hs), Cb, Cr)
MDJ_HD int64_t mdj_keep_source_offset(const MdjEncCrop& c, int mx, int my, int k) {
    const int luma = c.hs * c.vs;
    const int64_t mcus = int64_t(c.mcus_x) * c.mcus_y;
    if (k < luma) {
        const int kx = c.hs == 2 ? k & 1 : 0, ky = c.hs == 2 ? k >> 1 : k;
        return ((int64_t(my) * c.vs + ky) * (int64_t(c.mcus_x) * c.hs) + int64_t(mx) * c.hs + kx) * 64;
    }
    return (mcus * (luma + (k - luma)) + int64_t(my) * c.mcus_x + mx) * 64;
}

#endif  // MDJPEG_KEEP_H
