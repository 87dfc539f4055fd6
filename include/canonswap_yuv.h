/* canonswap_yuv.h -- 4:2:0 frames <-> the engine's RGB frames, on the device: the colour conversion between a codec and the chain.
 *
 * Why a header of its own: include/canonswap_hip.h is version 4 of the C ABI and is recorded line for line (tests/golden/abi_v4.txt, with the
 * binding table canonswap_amd/_lib.py ABI pinned entry by entry).  These entry points are an addition beside it, as those of
 * include/canonswap_landmarks.h are: the same library, the same cs_engine, the same conventions (0 or non-zero with cs_last_error(), caller-owned
 * contiguous device buffers, everything enqueued on the caller's stream, last parameter `void* stream`), and a version of their own,
 * cs_yuv_abi_version().  Their binding is canonswap_amd/_lib.py ABI_YUV.
 *
 * Decoders and encoders speak 4:2:0 YUV (ffmpeg's rawvideo yuv420p and nv12, every hardware decoder); the chain crops from and pastes into
 * (F, Ho, Wo, 3) uint8 RGB.  The reference lets swscale convert on the host on both sides (imageio-ffmpeg asked for rgb24; images2video,
 * src/utils/video.py) and so carries 3 bytes per pixel over the link where the codec has 1.5.  With these two calls the frames cross the link
 * as the codec has them.
 *
 * A frame is 3 Ho Wo / 2 bytes, Ho and Wo even: the Y plane (Ho x Wo), then
 *     layout 0, NV12            Ho / 2 rows of Wo bytes: U and V interleaved, U first
 *     layout 1, I420 (yuv420p)  the U plane (Ho / 2 x Wo / 2), then the V plane
 * which is ffmpeg's rawvideo layout of either format; F frames follow each other without padding.  Chroma is sited at the centre of its 2 x 2
 * block: it is replicated to the block's four pixels on the way in (what OpenCV's cvtColor and swscale's unscaled path do), and formed from
 * the sums of R, G and B over the four pixels on the way out.
 *
 * matrix 0: BT.601 (Kr 0.299, Kb 0.114); matrix 1: BT.709 (Kr 0.2126, Kb 0.0722).  full_range 0: Y 16 - 235, chroma 16 - 240; 1: 0 - 255.
 *
 * The arithmetic is integer: the real coefficients follow from Kr, Kb and the range scales in float64 (limited range: sy = 255 / 219,
 * sc = 255 / 224, y0 = 16; R = sy (Y - y0) + 2 (1 - Kr) sc (V - 128), B = sy (Y - y0) + 2 (1 - Kb) sc (U - 128), G from the chroma terms
 * 2 Kb (1 - Kb) / Kg and 2 Kr (1 - Kr) / Kg; the encode is the inverse matrix) and are rounded to 14 fractional bits for the decode and 16 for
 * the encode, whose chroma coefficients apply to the four-pixel sums (a shift of 18) and are adjusted so that each of the U and V triples sums
 * to exactly zero: a grey stays neutral.  Every result is (sum + half) >> shift, arithmetic, clamped to 0 .. 255.  The host builds the integers
 * in one place (canonswap_amd/csrc/yuv_math.h) and the kernels take them as arguments; tests/yuv_ref.py restates all of it in numpy and is
 * the definition: the kernels equal it bit for bit, and it lies within 1 LSB of the standards' float64 formula.  Parity with swscale's own
 * tables is not pinned (no ffmpeg or OpenCV where this is tested).
 *
 * Neither call uses engine scratch or synchronises; every argument is checked before anything is launched.  F >= 1, not bound by max_batch;
 * Ho and Wo even, 2 to 16384; every offset is 64-bit.  rgb and yuv must not overlap.  Buffers may start at any address and Wo may be any even
 * number: the fast path (8-byte accesses) needs both buffers 8-byte aligned and Wo a multiple of 8 (NV12) or 16 (I420); everything else takes
 * byte accesses with the same values.
 */
#ifndef CANONSWAP_YUV_H
#define CANONSWAP_YUV_H
#include <stdint.h>
#include "canonswap_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CS_YUV_ABI_VERSION 1   /* bumped whenever an entry point's meaning, the layouts or the arithmetic change */
int cs_yuv_abi_version(void);

/* F frames of 4:2:0 -> rgb (F x Ho x Wo x 3 uint8): pixel (y, x) from Y[y][x] and the U, V of block (y / 2, x / 2). */
int cs_yuv_to_rgb(cs_engine* e, int F, const uint8_t* yuv, int Ho, int Wo, int layout, int matrix, int full_range, uint8_t* rgb, void* stream);

/* The inverse: Y per pixel, U and V per 2 x 2 block from the sums of its R, G and B.
 *   keep 0   yuv is written only and never read.
 *   keep 1   yuv is an input as well: a block keeps its six bytes (four Y, U, V) if all four of its RGB pixels equal what those bytes decode
 *            to under the same layout, matrix and full_range (cs_yuv_to_rgb's arithmetic); every other block is re-encoded whole.  So
 *            cs_yuv_to_rgb, any writes to the RGB frames, cs_rgb_to_yuv(keep = 1) back into the buffer the frames came from leaves every
 *            block that was not written with the bytes it came in with: the untouched part of a frame is lossless, whatever the codec's
 *            values were (out-of-range ones, which clamp in RGB, included).  The rule is per block and knows nothing of faces. */
int cs_rgb_to_yuv(cs_engine* e, int F, const uint8_t* rgb, int Ho, int Wo, int layout, int matrix, int full_range, int keep, uint8_t* yuv,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
