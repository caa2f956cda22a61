/* msclip_color.h -- the colour stage of the training input path (msclip_amd/pairs.py, msclip_amd/color_hip.py): colour jitter,
 * random grayscale and Gaussian blur of a batch of uint8 images that msclip_resized_crop (msclip_input.h) wrote as out_u8, followed
 * by that call's per-channel table look-up.
 *
 * A header of its own, versioned on its own (MSCLIP_COLOR_ABI_VERSION, msclip_color_abi_version) and bound by a module of its own
 * (msclip_amd/color_hip.py, which opens the same libmsclip_hip.so): msclip_hip.h, the msclip_ext*.h headers, msclip_input.h and
 * the binding table of msclip_amd/hip.py stay as they are.
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules).
 *
 * THE ARITHMETIC.  The stages run in this order on the uint8 RGB image [H, W, 3], already flipped: 1 jitter, 2 grayscale, 3 blur,
 * 4 the table look-up lut[ch][p].  Every stage maps uint8 to uint8 (PIL rounds after every step: that is part of the definition).
 * Every fp32 operation is a single IEEE operation: no fused multiply-add, no fast-math.
 *   gray value   L(r, g, b) = (19595 r + 38470 g + 7471 b + 32768) >> 16, in integers.
 *   blend        blend(d, x, f), per channel, fp32, two roundings: t = d + f * (x - d); 0 if t <= 0, 255 if t >= 255, else trunc(t).
 *   jitter ops   brightness f: blend(0, x, f).  saturation f: blend(L(pixel), x, f).
 *                contrast f: blend(m, x, f) with m = floor(SUM L / (H W) + 0.5): SUM L is the exact integer sum over the image AS IT
 *                STANDS WHEN CONTRAST'S TURN COMES (after the ops that precede it in this image's order); the quotient is fp64.
 *                hue, shift q (0 ... 255): RGB -> HSV (8 bit) -> h = (h + q) & 255 -> RGB, with PIL's conversions:
 *     RGB -> HSV   v = max.  max == min: h = s = 0.  Otherwise cr = float(max - min), s = cr / float(max) (fp32),
 *                  rc = float(max - r) / cr, gc and bc likewise (fp32); hh = fp32(bc - gc) if r == max, else fp32(2.0 + rc - bc in
 *                  fp64) if g == max, else fp32(4.0 + gc - rc in fp64); hh = fp32(fmod(hh / 6.0 + 1.0, 1.0) in fp64);
 *                  h = clamp(int(double(hh) * 255.0), 0, 255), s8 = clamp(int(double(s) * 255.0), 0, 255).
 *     HSV -> RGB   s8 == 0: r = g = b = v.  Otherwise, all fp32: fh = float(h) * 6 / 255, fs = float(s8) / 255, i = floor(fh),
 *                  f = fh - i, p = v (1 - fs), q' = v (1 - fs f), t = v (1 - fs (1 - f)), each rounded
 *                  clamp(floor(double(x) + 0.5), 0, 255); (r, g, b) by i % 6: (v,t,p) (q',v,p) (p,v,t) (p,q',v) (t,p,v) (v,p,q').
 *   grayscale    r = g = b = L(pixel).
 *   blur         seven fp32 weights w0 ... w6 per image arrive as data (the host: w_k = exp(-k^2 / 2 sigma^2) / (w0 + 2 SUM_{k>=1}
 *                w_k) in fp64, rounded once; sigma <= 2, radius 6 = ceil(3 * 2) for every image).  Separable, horizontal pass
 *                first.  Per pass and channel acc = SUM_{k=-6..6} w_|k| x[mirror(i + k)], over ascending k in fp32 from 0, no fma;
 *                each pass is rounded clamp(floor(acc + 0.5), 0, 255) (an acc that is not a number gives 0).
 *                mirror(j, n): 0 for n == 1; otherwise m = 2 (n - 1), j = ((j mod m) + m) mod m, and m - j where j >= n:
 *                reflection without repeating the edge, for any overrun.  The border is mirrored, so flip-then-blur equals
 *                blur-then-flip: working on the already flipped image is exact.
 * A numpy restatement of this text (tests/color_ref.py) equals PIL bit for bit on convert("L"), ImageEnhance.Brightness / Contrast /
 * Color, convert("HSV") and back; the blur differs from an fp64 mirror correlation by at most one level on a few values per million. */
#ifndef MSCLIP_COLOR_H
#define MSCLIP_COLOR_H

#ifdef __cplusplus
extern "C" {
#endif

/* The radius of the blur: 13 taps per pass, MSCLIP_COLOR_RADIUS halo rows on each side of a band. */
#define MSCLIP_COLOR_RADIUS 6
/* The LDS budget of one workgroup of the band kernel in bytes (dynamic LDS, as for msclip_resized_crop).  A workgroup of a blurred
 * image holds, for a band of `band` output rows,
 *     the pointwise chain's result    (band + 12) x W pixels, uint8 RGB in one dword each     4 (band + 12) W
 *     the horizontal pass's result    (band + 12) x W pixels, likewise                        4 (band + 12) W
 * that is 8 (band + 12) W bytes.  The band is the largest of 32, 24, 16, 12, 8, 6, 4, 3, 2, 1 (capped at H) that fits; a call whose
 * band of ONE row does not fit (W > 630) is rejected, whatever `stages` says.  At 224 x 224: band 24, 64 512 B.  A launch whose
 * `stages` has no blur bit allocates no LDS. */
#define MSCLIP_COLOR_LDS_BYTES 65536

/* The band (output rows of a workgroup) and the dynamic LDS bytes of a blurring launch for these extents; -1 where the call would be
 * rejected for them.  Host arithmetic only. */
int msclip_color_augment_band(int H, int W);
int msclip_color_augment_lds(int H, int W);

/* Jitter, grayscale, blur and table look-up (the arithmetic above) of B images.
 *   src_u8  uint8 [B, H, W, 3]
 *   ops     int32 [B, 8]: order[0..3] (0 brightness, 1 contrast, 2 saturation, 3 hue, applied left to right; anything else is
 *           skipped, and so is the second occurrence of an op), the hue shift (taken & 255), the gray flag, the blur flag (each
 *           "not 0"), one reserved entry
 *   coef    fp32 [B, 12]: f_b, f_c, f_s, one pad, w0 ... w6, one pad
 *   lut     fp32 [3, 256]: the value of channel c at pixel level v
 *   stages  a host bit mask, jitter 1, gray 2, blur 4: what the launch has to provide for.  The per-image entries of `ops` then
 *           decide per image; a stage whose bit is clear is off for every image, whatever `ops` says.
 *   work    int32 [B]: scratch for the contrast means.  May be NULL when stages & 1 is 0.
 *   out     [B, 3, H, W], fp32, or bf16 (out_bf16 != 0: round-to-nearest-even of the fp32 value)
 *   out_u8  uint8 [B, H, W, 3], the augmented pixels; optional (NULL: not stored)
 * ops and coef are device data, so the kernels guard them: a factor that is not finite counts as 1, a factor is clamped to [0, 4];
 * a weight that is not finite counts as 0.
 * With the jitter bit set, a first kernel runs one workgroup per image: it applies the ops that precede contrast to every pixel in
 * registers, sums L as 64-bit integers (a fixed tree, no atomics, nothing to zero) and writes m to work[b].  A second kernel runs
 * B x ceil(H / band) workgroups: one image and one band of rows each.  For an image whose blur flag is set it runs the pointwise
 * chain over the band's rows and 6 mirrored halo rows on each side into LDS, the horizontal pass into a second LDS buffer, then the
 * vertical pass; for any other image it runs the chain and stores.  Nothing intermediate but `work` goes to HBM; every output has
 * one writer and every sum a fixed order: bitwise repeatable.
 * Rejected: src_u8, ops, coef, lut or out NULL; work NULL with stages & 1; ops, coef, lut, work or out not 4-byte aligned (out
 * 2-byte for bf16); B, H or W <= 0; stages outside 0 ... 7; out_u8 == src_u8 (the blur reads neighbours); a band of one row over
 * the LDS budget; B * ceil(H / band) above 2^31 - 1.
 * Device pointers only: recordable in a launch plan. */
int msclip_color_augment(const void* src_u8, const int* ops, const float* coef, const float* lut, int B, int H, int W, int stages,
                         void* work, void* out, int out_bf16, void* out_u8, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_COLOR_ABI_VERSION 1
int msclip_color_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
