/*
 * glass_hip_feature_roimask.h — entry points of libglass_hip.so (gfx950): mask polygons straight from the RoI masks.
 *
 * One header per feature: glass_hip.h, glass_hip_ext.h and the set of glass_hip_ext_<feature>.h headers are closed (the host
 * tests pin them), so this one is include/glass_hip_feature_<feature>.h.  It includes the first; the binding parses every
 * such header (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for
 * sizes, 0 or a negative GLASS_E* code (glass_last_error() has the message), all work enqueued on the caller's stream,
 * nothing synchronises.  glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_ROIMASK_H
#define GLASS_HIP_FEATURE_ROIMASK_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E*, glass_mask_rings_workspace_bytes, glass_mask_rings_write */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ mask polygonisation without the pasted masks
 * glass_paste_rotated_masks followed by glass_mask_windows / glass_mask_rings_count, without the uint8 [R][H][W] tensor
 * between them: masks [R][M][M] float (probabilities), boxes [R][5] (cx, cy, w, h, angle in degrees, image pixels).  Pixel
 * (x, y) of mask r is set iff the paste's value there (the arithmetic of glass_paste_rotated_masks, operation for operation:
 * one device function serves both) is >= threshold.  That is evaluated where a stage needs it and stored nowhere.
 *
 * The candidate rectangle of a box: with A = |w|/2 (1 + 1/M), B = |h|/2 (1 + 1/M), ex = A|cos| + B|sin|, ey = A|sin| + B|cos|
 * (double), the pixels whose centres lie in [c - e, c + e], widened by 2 pixels on every side and clipped to the image; the
 * paste cannot set a pixel outside it.  Empty (x1 < x0) for a box with a non-finite component, for which the paste sets
 * nothing either.  It is computed on the device from the box, and clipped before anything of it becomes an integer.
 * Limit: the 2-pixel margin covers the paste's float32 rounding while one float32 ulp of |cx|, |cy|, |w|, |h| stays well below
 * a pixel (values up to about 2^20, i.e. boxes at image scale, as the detector's post-processing leaves them).  For boxes far
 * beyond that the float32 paste may set pixels outside the float64 rectangle: the windows may then be too small and the rings
 * differ from the two-step path.  Memory safety does not depend on the margin (everything is clipped before it is an index).
 *
 * glass_roi_mask_rects: rects int32 [R][4] (16-byte aligned) = that rectangle, x0, y0, x1, y1 inclusive.  Not needed by
 *   the other two (they compute it themselves); for callers and tests that want to see it.  One launch.
 * glass_roi_mask_windows: windows int32 [R][4] (16-byte aligned), what glass_mask_windows gives for the pasted masks: the
 *   tight rectangle of the set pixels, x1 < x0 for an empty mask.  Evaluates the predicate over the candidate rectangles only.
 *   Two launches.
 * glass_roi_mask_rings_count: glass_mask_rings_count with the predicate in place of the byte in its first labelling stage;
 *   every other stage, the workspace layout (size it with glass_mask_rings_workspace_bytes from a host copy of the windows),
 *   ring_off and status are those of glass_mask_rings_count.  Follow it with glass_mask_rings_write, which serves both forms.
 * Needs R >= 0, 1 <= M <= 4096, H, W in 1..65535 with H * W < 2^31, threshold > 0 (at 0 or below the paste sets the whole
 * image or is its visualisation mode) and non-null pointers unless R == 0 (then nothing is launched); anything else returns a
 * negative code before any launch.  Integer atomics only; bit-identical from run to run and to the two-step path.           */
int glass_roi_mask_rects(const float* boxes, int R, int M, int H, int W, int* rects, glass_stream_t stream);
int glass_roi_mask_windows(const float* masks, const float* boxes, int R, int M, int H, int W, float threshold, int* windows,
                           glass_stream_t stream);
int glass_roi_mask_rings_count(const float* masks, const float* boxes, int R, int M, int H, int W, float threshold,
                               const int* windows, void* workspace, int64_t workspace_bytes, int* ring_off, int* status,
                               glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_ROIMASK_H */
