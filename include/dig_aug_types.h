/* dig_aug_types.h -- layout of the per-image parameter table of the MoCo key-view augmentation (dataset/dataset_image.py:39-50,88-120,
 * 145-149 of the reference: imgaug SomeOf((2, 5), 10 seqCLR ops) at the crop's resolution, Resize((32, 128), BICUBIC),
 * RandomApply([ColorJitter(0.4, 0.4, 0.2, 0.1)], p=0.8), RandomGrayscale(p=0.2), ToTensor + Normalize).  Types only: the entry points
 * are in dig_hip.h, the semantics of every field in dig_amd/csrc/keyview.inc.
 *
 * One table of DIG_KV_WORDS 32-bit words per image.  The sampler fills the raw draws AND the coefficients derived from them for the
 * image's height / width; the kernels read only the fields their op needs.  A hand-built table (tests) must fill both.
 *   op ids: 0 LinearContrast, 1 GaussianBlur, 2 Crop top/bottom, 3 Crop left/right, 4 Sharpen, 5 Rotate, 6 PiecewiseAffine,
 *           7 PerspectiveTransform, 8 Solarize, 9 Grayscale(alpha)
 *   jitter op ids: 0 brightness, 1 contrast, 2 saturation, 3 hue
 */
#ifndef DIG_AUG_TYPES_H
#define DIG_AUG_TYPES_H

#define DIG_KV_WORDS 128
#define DIG_KV_MAX_OPS 5
#define DIG_KV_MAX_TAPS 11 /* GaussianBlur: radius ceil(3 sigma) <= 5 for sigma <= 1.5 */

typedef struct dig_kv_params {
  /* ---- stage A: the op sequence */
  int n_ops;                 /* 0..5 (the sampler draws 2..5) */
  int ops[DIG_KV_MAX_OPS];   /* op ids in the order they run; entries at and after n_ops are -1 */
  /* ---- stage A: raw draws */
  float contrast_alpha;      /* op 0: U(0.5, 1) */
  float blur_sigma;          /* op 1: U(0.5, 1.5) */
  float crop_tb[2];          /* op 2: top, bottom fraction, U(0, 0.3) each */
  float crop_lr[2];          /* op 3: left, right fraction, U(0, 0.1) each */
  float sharpen_alpha;       /* op 4: U(0, 0.5) */
  float sharpen_lightness;   /* op 4: U(0, 0.5) */
  float rotate_deg;          /* op 5: U(-10, 10) */
  float pa_scale;            /* op 6: U(0.03, 0.04) */
  float pa_dy[16];           /* op 6: N(0, s) * H per control point, row-major over the 4 x 4 grid */
  float pa_dx[16];           /* op 6: N(0, s) * W */
  float persp_sigma;         /* op 7: U(0.05, 0.1) */
  float persp_d[8];          /* op 7: |N(0, sigma)| for TL.x TL.y TR.x TR.y BR.x BR.y BL.x BL.y (fractions of W / H, moved inward) */
  float solar_tau;           /* op 8: U(32, 128) */
  int solar_above;           /* op 8: 1 = invert v >= tau, 0 = invert v < tau */
  float gray_alpha;          /* op 9: U(0, 1) */
  /* ---- stage A: coefficients derived for this image's H x W */
  int blur_radius;           /* op 1: ceil(3 sigma) */
  float blur_taps[DIG_KV_MAX_TAPS]; /* op 1: normalised Gaussian taps, index radius + d for offset d */
  float sharpen_k[9];        /* op 4: 3 x 3 kernel, row-major */
  int crop_y[2];             /* op 2: first kept row, kept rows (>= 1) */
  int crop_x[2];             /* op 3: first kept column, kept columns (>= 1) */
  float rot[6];              /* op 5: source (x, y) = (rot0 x + rot1 y + rot2, rot3 x + rot4 y + rot5) */
  float homog[9];            /* op 7: source = ((h0 x + h1 y + h2) / (h6 x + h7 y + h8), (h3 x + h4 y + h5) / (...)) */
  /* ---- stage B */
  int jitter;                /* 1 with p = 0.8: ColorJitter runs */
  int jit_order[4];          /* permutation of the four jitter ops (an entry outside 0..3 is skipped: hand-built tables) */
  float jit_factor[4];       /* brightness U(0.6, 1.4), contrast U(0.6, 1.4), saturation U(0.8, 1.2), hue U(-0.1, 0.1) */
  int hue_shift;             /* trunc(hue * 255) mod 256 (hue as a double, as torchvision's float(...) hands it to numpy) */
  int gray;                  /* 1 with p = 0.2: RandomGrayscale */
  int pad[17];
} dig_kv_params;

#ifdef __cplusplus
static_assert(sizeof(dig_kv_params) == DIG_KV_WORDS * 4, "dig_kv_params is DIG_KV_WORDS words");
#endif

#endif /* DIG_AUG_TYPES_H */
