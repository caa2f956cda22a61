/* msclip_input.h -- the training input path (msclip_amd/pairs.py, msclip_amd/input_hip.py): one launch that turns a staged batch
 * of decoded images into network input -- crop, antialiased resize, horizontal flip and normalisation.
 *
 * A header of its own, versioned on its own (MSCLIP_INPUT_ABI_VERSION, msclip_input_abi_version) and bound by a module of its own
 * (msclip_amd/input_hip.py, which opens the same libmsclip_hip.so): msclip_hip.h, msclip_ext.h ... msclip_ext5.h and the binding
 * table of msclip_amd/hip.py stay as they are.
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules). */
#ifndef MSCLIP_INPUT_H
#define MSCLIP_INPUT_H

#ifdef __cplusplus
extern "C" {
#endif

/* The largest ratio of a slot extent to the output extent, per axis, that msclip_resized_crop takes: a crop box lies inside its
 * image and the image inside its slot, so no box is scaled down by more than this. */
#define MSCLIP_CROP_MAX_SCALE 8
/* The LDS budget of one workgroup of msclip_resized_crop in bytes (dynamic LDS; a CU of gfx950 has 160 KiB, so two workgroups
 * stay resident at the full budget).  It holds, for a band of `band` output rows and the worst scale the slot allows
 * (sx = max(slot_w / out_w, 1), sy likewise, S = 1 bilinear / 2 bicubic, KX = 2 ceil(S sx) + 1, KY = 2 ceil(S sy) + 1,
 * ROWS = floor((band - 1) slot_h / out_h + 2 S sy) + 2):
 *     horizontal taps   out_w x (KX fp32 weights + first column + count)       4 out_w (KX + 2)
 *     vertical taps     band x (KY fp32 weights + first row + count)           4 band (KY + 2)
 *     intermediate      ROWS x out_w pixels of the horizontal pass, uint8 RGB in one dword each     4 ROWS out_w
 * The band is the largest of 32, 24, 16, 12, 8, 6, 4, 3, 2, 1 (capped at out_h) that fits; a call whose band of ONE row does not
 * fit is rejected.  At 512 x 512 slots and 224 x 224 bicubic output: KX = KY = 11, band 16, 52 800 B. */
#define MSCLIP_CROP_LDS_BYTES 65536

/* The band (output rows of a workgroup) and the dynamic LDS bytes that msclip_resized_crop uses for these extents; -1 where the
 * call would be rejected for them.  Host arithmetic only. */
int msclip_resized_crop_band(int slot_h, int slot_w, int out_h, int out_w, int filter);
int msclip_resized_crop_lds(int slot_h, int slot_w, int out_h, int out_w, int filter);

/* PIL's Image.crop(box).resize((out_w, out_h), filter) of B staged images, then an optional horizontal flip and a per-channel table
 * look-up, in one launch.
 *   src     uint8, B slots of [slot_h, slot_w, 3] (HWC); image b is anchored at its slot's top-left, row pitch slot_w * 3
 *   dims    int32 [B, 2]: (h, w) of image b            boxes   int32 [B, 4]: (top, left, height, width) inside dims
 *   flip    int32 [B] or NULL                          lut     fp32 [3, 256]: the value of channel c at pixel level v
 *   filter  2 = bilinear (triangle), 3 = bicubic (a = -0.5): PIL's codes
 *   out     [B, 3, out_h, out_w], fp32, or bf16 (out_bf16 != 0: round-to-nearest-even of the fp32 value)
 *   out_u8  uint8 [B, out_h, out_w, 3], the resampled pixels; optional (NULL: not stored)
 * Per axis, box extent n and output extent m, all fp32: scale = n / m, fs = max(scale, 1), sup = S fs; for output index i,
 * c = (i + 0.5) scale, lo = max(0, int(c - sup + 0.5)), hi = min(n, int(c + sup + 0.5)), w_k = f((k + lo - c + 0.5) / fs) divided by
 * the sum of the w_k: taps never leave the crop box.  Two passes, the horizontal one first; its result is rounded and clamped to
 * uint8 (clamp(floor(x + 0.5), 0, 255)) before the vertical pass, whose result p is rounded the same way (PIL's own arithmetic:
 * the uint8 intermediate is part of the definition).  out_u8[b][y][x'][ch] = p, out[b][ch][y][x'] = lut[ch][p], with x' = x, or
 * x' = out_w - 1 - x where flip[b] != 0: a flipped result is bitwise the unflipped one with its columns reversed.
 * Sums run over ascending k in fp32 without fused multiply-add; every output has one writer: bitwise repeatable.
 * A workgroup takes one sample and one band of output rows (grid = B x ceil(out_h / band)); the taps and the intermediate rows
 * live in LDS (MSCLIP_CROP_LDS_BYTES), nothing intermediate goes to HBM.
 * dims and boxes are device data, so the host cannot check them: the kernel clamps dims into the slot (1 <= h <= slot_h,
 * 1 <= w <= slot_w) and the box into dims (0 <= top < h, 1 <= height <= h - top, columns likewise) before it indexes anything.
 * Rejected: src, dims, boxes, lut or out NULL; dims, boxes, flip, lut or out not 4-byte aligned (out 2-byte for bf16); B <= 0;
 * out_h <= 0 or out_w <= 0; slot_h <= 0 or slot_w <= 0; filter not 2 or 3; slot_h > MSCLIP_CROP_MAX_SCALE * out_h or slot_w >
 * MSCLIP_CROP_MAX_SCALE * out_w; a band of one row over the LDS budget; B * ceil(out_h / band) above 2^31 - 1.
 * Device pointers only: recordable in a launch plan. */
int msclip_resized_crop(const void* src, int slot_h, int slot_w, const int* dims, const int* boxes, const int* flip,
                        const float* lut, int B, int filter, int out_h, int out_w, void* out, int out_bf16, void* out_u8,
                        void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_INPUT_ABI_VERSION 1
int msclip_input_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
