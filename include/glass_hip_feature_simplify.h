/*
 * glass_hip_feature_simplify.h — entry points of libglass_hip.so (gfx950): exact Douglas-Peucker simplification of traced rings.
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_SIMPLIFY_H
#define GLASS_HIP_FEATURE_SIMPLIFY_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ ring simplification
 * Input: the rings as glass_mask_rings_write leaves them, xy int32 [n_points][2] (8-byte aligned) and ring_off int32
 * [n_rings + 1]; ring r is xy[ring_off[r] .. ring_off[r + 1]), closed (last point == first) or open, possibly empty.
 * The statement is glass_amd.evaluation.ring_simplify.simplify_ring, which the kernels equal vertex for vertex.  With
 * v[0..n-1] the ring without its closing duplicate and q4 = 4 * tolerance (an integer, 0..4096, i.e. quarter pixels):
 *   distance of p from the chord (a, b): d = b - a, w = p - a, L = d.d, t = w.d; num = |w|^2 L if t <= 0, |p - b|^2 L if
 *     t >= L, (d x w)^2 otherwise (squared distance to the segment, times L); for a == b, L = 1 and num = |w|^2.  "Farther
 *     than the tolerance" is 16 num > q4^2 L.
 *   anchors: A = v[0]; B = the vertex of largest |v[i] - A|^2, lowest index on a tie.
 *   Douglas-Peucker on the chains A..B and B..v[n-1], A: the interior vertex of largest num (earliest in chain order on a tie)
 *     is kept if it is farther than the tolerance and both halves are processed; otherwise the interior is dropped.
 *   third vertex: if only A and B survive, the vertex of largest num against the chord (A, B) is kept too if that num > 0
 *     (lowest index on a tie); a ring of zero area becomes A, B.
 *   n <= 3, or every vertex equal to A: the ring is kept as it is.  An empty ring stays empty.  A closed ring is closed again.
 * Exactness: |coordinate| <= 2^20 (the bound of glass_ring_check), so L < 2^44, 16 num < 2^90 and q4^2 L < 2^68: every
 * product is an exact 64 x 64 -> 128 bit unsigned product and every comparison a 128-bit one.  There is no floating point.
 * Determinism: one wavefront owns one ring; the split of a chain is one 64-lane arg-max by (num, earliest position), a total
 * order, so it does not depend on the reduction's shape; pending chains wait on a stack of 64 entries, which the rule
 * "continue with the shorter half, push the longer" bounds by log2(2^31) + 1 = 32.  No atomics but the status (an integer
 * maximum).  Two runs are bit-identical.
 * A ring of at most GLASS_RING_SIMPLIFY_LDS_POINTS points (with its closing duplicate) is staged in LDS, a longer one is read
 * from global memory by the same code.
 *
 * glass_ring_simplify_workspace_bytes: bytes of the workspace (16-byte aligned) for these sizes; negative for bad sizes.
 * glass_ring_simplify_mark: one keep flag per input point into the workspace, and out_off int32 [n_rings + 1], the running sum
 *   of the kept counts (the ring_off of the result), as glass_mask_rings_count fills ring_off.  status (one int32, written
 *   here): 0, or the largest of 1 = a coordinate beyond 2^20 in magnitude, 2 = an offset that decreases or leaves
 *   0..n_points, 3 = chain stack exhausted (cannot happen below 2^31 points).  The kernels do not trust their input: a ring
 *   with a bad offset or coordinate is skipped, nothing is read outside xy, and with a non-zero status out_off is all zeros.
 *   Two launches.
 * glass_ring_simplify_write: out_xy int32 [n_out][2] (n_out = out_off[n_rings], read back by the caller), the kept points in
 *   ring order.  Same xy, ring_off and workspace as the mark call.  One launch.
 * Needs 0 <= n_points < 2^31, n_rings >= 0, 0 <= q4 <= 4096 and non-null pointers; anything else returns a negative code
 * before any launch.  n_rings == 0 launches nothing; n_points == 0 launches nothing either (ring_off is not read, out_off
 * and status are cleared by a memset).                                                                                      */
#define GLASS_RING_SIMPLIFY_LDS_POINTS 4096
int64_t glass_ring_simplify_workspace_bytes(int64_t n_points, int n_rings);
int glass_ring_simplify_mark(const int* xy, int64_t n_points, const int* ring_off, int n_rings, int q4, void* workspace,
                             int64_t workspace_bytes, int* out_off, int* status, glass_stream_t stream);
int glass_ring_simplify_write(const int* xy, int64_t n_points, const int* ring_off, int n_rings, const void* workspace,
                              int64_t workspace_bytes, const int* out_off, int* out_xy, int64_t n_out, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_SIMPLIFY_H */
