/*
 * glass_hip_feature_rotate.h — entry points of libglass_hip.so (gfx950): an image rotated as Pillow rotates it, and rotated boxes
 * moved by the same matrix.
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_ROTATE_H
#define GLASS_HIP_FEATURE_ROTATE_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ the rotated image
 * The statement is glass_amd.data.transforms.rotate_u8_host (numpy float64), which equals
 * PIL.Image.rotate(angle, resample=BILINEAR, expand=True, fillcolor=fill) on a uint8 RGB image byte for byte; the kernel equals
 * the statement byte for byte.  The host (glass_amd.data.transforms.RotationTransform) makes the matrix and the output size
 * as Pillow makes them, in Python floats; the six doubles come here as they are and map OUTPUT to INPUT.
 *
 * src uint8 [H][W][3], dst uint8 [Ho][Wo][3], both dense.  kind:
 *   0  the copy:             dst[y][x] = src[y][x],                  Ho = H, Wo = W
 *   1  90 degrees (ccw):     dst[y][x] = src[x][W - 1 - y],          Ho = W, Wo = H
 *   2  180 degrees:          dst[y][x] = src[H - 1 - y][W - 1 - x],  Ho = H, Wo = W
 *   3  270 degrees:          dst[y][x] = src[H - 1 - x][y],          Ho = W, Wo = H
 *      (Pillow's transpose shortcuts at angle % 360 = 0, 90, 180, 270; the matrix is not used)
 *   4  the affine bilinear form.  For the output pixel (x, y), with m = matrix6 and every product and sum below a float64
 *      operation of its own, rounded on its own, in this order (no fused multiply-add: one would change the last bit of a
 *      coordinate or of v, and with it an inside / outside decision or a byte):
 *        xin = m0 * (x + 0.5) + m1 * (y + 0.5) + m2,   yin = m3 * (x + 0.5) + m4 * (y + 0.5) + m5
 *        unless 0 <= xin < W and 0 <= yin < H (a value that is not a number fails this): the three fill bytes.
 *        xin -= 0.5, yin -= 0.5; x0 = floor(xin), y0 = floor(yin); dx = xin - x0, dy = yin - y0
 *        columns clip(x0) and clip(x0 + 1) into [0, W - 1], row clip(y0) into [0, H - 1]; per channel, with a and b the two
 *        bytes of a row:  v1 = a + (b - a) * dx;  v2 the same on row y0 + 1 if 0 <= y0 + 1 < H, otherwise v2 = v1;
 *        v = v1 + (v2 - v1) * dy;  the byte is v truncated (v lies in [0, 255]).
 *
 * matrix6_host: six doubles on the HOST, read before the call returns.  fill_r, fill_g, fill_b: the bytes of channels 0, 1, 2
 * outside the source.
 *
 * Validated before any launch, GLASS_EINVAL otherwise: H, W, Ho, Wo >= 0; H * W * 3 and Ho * Wo * 3 below 2^31; kind in 0..4;
 * for kind 0..3 the output size the kind implies; matrix6_host non-null and its six entries finite; the fill in 0..255; src and
 * dst non-null unless H * W == 0 or Ho * Wo == 0, in which case nothing is launched (and nothing written).
 *
 * One launch.  A workgroup takes a compact 32 x 32 tile of the output, a wavefront 32 x 8 pixels of it, so that a wavefront's
 * source footprint is a small rotated rectangle at any angle; a thread makes four neighbouring pixels of a row and stores
 * them as three whole dwords wherever the twelve bytes lie inside the row (the groups are laid out per row so that they
 * start on a dword of dst, whatever the row length and the alignment of dst), single bytes at the two ends of a row.  Every
 * source index is clipped into the image before it is used, and a byte is written only for 0 <= x < Wo, 0 <= y < Ho: nothing is
 * read outside src or written outside dst.  Every output byte is written by exactly one thread from values that depend on its
 * position alone: two runs are bit-identical.                                                                              */
int glass_rotate_u8(const uint8_t* src, int H, int W, uint8_t* dst, int Ho, int Wo, const double* matrix6_host, int kind,
                    int fill_r, int fill_g, int fill_b, glass_stream_t stream);

/* ------------------------------------------------------------------ rotated boxes through the same matrix
 * The statement is glass_amd.data.transforms.RotationTransform.map_rotated_boxes (numpy float64).  boxes float [n][5] =
 * (cx, cy, w, h, a in degrees), out float [n][5] (may be boxes itself).  Every value is widened exactly to float64; with
 * m = matrix6_host (six doubles on the HOST: the direction to apply, INPUT to OUTPUT to follow the image, OUTPUT to INPUT to
 * come back) and without contraction:
 *   cx' = m0 * cx + m1 * cy + m2,  cy' = m3 * cx + m4 * cy + m5,  w and h kept,
 *   a' = a + theta_degrees, then a' - 360 * floor((a' + 180) / 360): into [-180, 180)
 * (the angle adds: a box's angle is counter-clockwise, as the image's rotation is; to come back pass -theta), each rounded to
 * float32 once.  A row with a value that is not finite is copied bit for bit.
 * One thread per box, one launch; n == 0 launches nothing.  n < 0 or above 2^26, a null pointer with n > 0, a null or non-finite matrix or a
 * non-finite theta return GLASS_EINVAL before any launch.  Row i depends on row i alone: two runs are bit-identical.       */
int glass_rotate_boxes(const float* boxes, int n, const double* matrix6_host, double theta_degrees, float* out,
                       glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_ROTATE_H */
