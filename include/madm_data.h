// C ABI of libmadm_data.so: the dataset pipeline's native part (madm_amd/data.py, madm_amd/png_read.py).
//
// A library of its own next to libmadm_hip.so: decoded 8-bit images go through ONE launch each on their way to a training
// or evaluation tensor, and the PNG reader's one hot loop (scanline unfiltering) runs here on the host.  Same style as
// madm_hip.h: raw pointers, explicit sizes and strides, a hipStream_t passed as void*, an int status, no allocation and
// no ownership transfer.  On failure the message is in mdata_last_error() (thread-local).
//
// The resizes are PIL's, bit for bit (Pillow Resample.c / Geometry.c for 8-bit images):
//   BILINEAR  two passes, horizontal first, uint8 in between; per output index a window [min, min + n) of the input and n
//             integer coefficients (int(0.5 + w * 2^22)); pixel = clip8((2^21 + sum pixel * coef) >> 22).
//   NEAREST   one index table per axis.
// The tables are built by the caller on the host in float64 (madm_amd/data.py: bilinear_table, nearest_table) and live on
// the device.  The kernels clamp every table entry to the source window, so no table content can make them read or write
// outside the buffers described by the arguments; a table that does not come from that recipe only gives other pixels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDATA_OK 0
#define MDATA_ERR_INVALID_ARG 1
#define MDATA_ERR_LAUNCH 2
#define MDATA_ERR_FORMAT 3          /* mdata_png_unfilter: a scanline's filter byte is not 0 .. 4 */

#define MDATA_MAX_TAPS 17           /* widest bilinear window: scale factors up to 8 (ceil(8) * 2 + 1) */

int mdata_abi_version(void);        /* 1 */
const char* mdata_last_error(void);

// uint8 HWC source window -> f32 [3, ch, cw], values 0 .. 255: PIL-exact bilinear resize of the window to (rh, rw), crop
// of (ch, cw) at (y0, x0) of the resized image, optional horizontal flip, gray -> 3 planes, cast.  Only the crop is computed.
//   src       device, uint8, any alignment: first byte of the window (pixel (0, 0), channel 0); C in {1, 3} interleaved
//             channels; src_ld = BYTES from one source row to the next (>= in_w * C).  in_h x in_w = the window.
//   hbounds   device, int32 [rw][2] = (first input column, taps), 4-byte aligned; hcoef device, int32 [rw][hk], 4-byte
//             aligned; hk in 1 .. MDATA_MAX_TAPS.  Both NULL (hk = 0) = the horizontal pass is skipped: requires rw == in_w.
//   vbounds, vcoef, vk   the same for rows ([rh][2], [rh][vk]); both NULL = skipped: requires rh == in_h.
//   out       device, f32, 4-byte aligned: element (p, y, x) at out[p * out_plane + y * out_ld + x]; out_ld >= cw,
//             out_plane >= ch * out_ld (elements).
//   flip      0 / 1: column x of the crop is stored at column cw - 1 - x.
int mdata_prep_image_u8(const uint8_t* src, int C, int src_ld, int in_h, int in_w,
                        const int32_t* hbounds, const int32_t* hcoef, int hk,
                        const int32_t* vbounds, const int32_t* vcoef, int vk,
                        int rh, int rw, int y0, int x0, int ch, int cw, int flip,
                        float* out, int out_ld, int out_plane, void* stream);

// uint8 label window -> int64 [ch, cw]: NEAREST resize to (rh, rw) through two index tables, crop at (y0, x0), optional
// flip, then lut1 (the DELIVER rule), then lut2 (label_convert), with a histogram of the crop between the two tables.
//   src       device, uint8, any alignment: pixel (y, x) at src[y * src_ld + x * src_px] (src_px = channels of an HWC
//             source, whose channel 0 is read; 1 for HW).  in_h x in_w = the window.
//   ytab      device, int32 [rh], 4-byte aligned, or NULL = identity (requires rh == in_h); xtab likewise ([rw], in_w).
//   lut1, lut2   device, uint8 [256], any alignment, or NULL = identity.
//   hist      device, int32 [256], 4-byte aligned, or NULL: hist[lut1[v]] += 1 for every pixel of the crop (atomic adds:
//             the caller zeroes it, on the same stream, before the launch).
//   out       device, int64, 8-byte aligned: element (y, x) at out[y * out_ld + x]; out_ld >= cw (elements).
int mdata_prep_label_u8(const uint8_t* src, int src_px, int src_ld, int in_h, int in_w,
                        const int32_t* ytab, const int32_t* xtab, int rh, int rw, int y0, int x0, int ch, int cw, int flip,
                        const uint8_t* lut1, const uint8_t* lut2, int32_t* hist,
                        int64_t* out, int out_ld, void* stream);

// HOST function: undoes the PNG scanline filters (types 0 .. 4: None, Sub, Up, Average, Paeth).
//   in        in_len bytes = height rows of (1 filter byte + row_bytes); in_len must equal height * (1 + row_bytes)
//   out       out_len bytes = height rows of row_bytes; out_len must equal height * row_bytes; must not overlap in
//   bpp       bytes per complete pixel, 1 .. 8 (the filters' left-neighbour distance)
// Any alignment.  Returns MDATA_ERR_INVALID_ARG on inconsistent lengths (nothing is read or written) and MDATA_ERR_FORMAT at
// the first row whose filter byte is above 4: the rows before it are decoded, that row and the rows behind it are not written.
int mdata_png_unfilter(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_len, int height, size_t row_bytes, int bpp);

#ifdef __cplusplus
}
#endif
