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


/* ---- the fine-tune ABINet augmentation (--num_view 2 --use_abi_aug; transforms.py:188-504 and dataset/dataset_lmdb.py:36-47 of the
 * reference): CVGeometry(45, (0, 0), (0.5, 2), (45, 15), 0.5, p 0.5), CVDeterioration(20, 6, 4, p 0.25), CVColorJitter(0.5, 0.5, 0.5, 0.1,
 * p 0.25), Resize((32, 128), BICUBIC), ToTensor, Normalize.  Semantics of every field: dig_amd/csrc/abiaug.inc.
 *
 * dig_abi_run: what the reference draws once per dataset object (CVGeometry / CVDeterioration constructors), fixed for a whole run.
 * dig_abi_params: one table of DIG_ABI_WORDS words per image, filled by dig_abiaug_sample (raw draws, the warp map, the warped size, the
 * motion-blur kernel and the image's workspace offset).  A hand-built table (tests) must fill all of them. */
#define DIG_ABI_WORDS 96
#define DIG_ABI_MB_MAX 5           /* motion-blur kernel size max(int(Beta(1,4) 6), 1) <= 5 */

typedef struct dig_abi_run {
  int geom_type;             /* 0 rotation, 1 affine, 2 perspective */
  int noise_var;             /* Gaussian noise variance, 1..19 */
  int mb_size;               /* motion-blur kernel size, 1..5 */
  float mb_angle;            /* motion-blur angle, degrees, U(-90, 90) */
  int rescale_factor;        /* pyrDown steps, 0..4 (0: the rescale op is the identity and is skipped) */
  int det_order[3];          /* the deterioration ops in the order they run: 0 noise, 1 motion blur, 2 rescale */
} dig_abi_run;

typedef struct dig_abi_params {
  int geom, det, jit;        /* the three gates (p 0.5, 0.25, 0.25) */
  int geom_interp;           /* 0 nearest, 1 linear, 2 cubic, 3 area (a warp treats area as linear) */
  float angle, scale;        /* rotation / affine angle sym(45) (degrees), affine scale U(0.5, 2) */
  float shear[2];            /* affine shear sym(45), sym(15) (degrees) */
  int persp_ow[4];           /* perspective corner offsets along x, int(Beta(1,4) 0.5 W / 2): TL TR BR BL */
  int persp_oh[4];           /* ... along y, int(Beta(1,4) 0.5 H / 2) */
  int h, w;                  /* the crop's size */
  int wh, ww;                /* the size after the geometry (h, w when geom == 0) */
  float minv[9];             /* warp map, output (x, y) -> source ((m0 x + m1 y + m2) / d, (m3 x + m4 y + m5) / d), d = m6 x + m7 y + m8 */
  int rs_interp[2];          /* rescale: interpolation of the resize to 128 x 512 and of the resize back (0..3 as geom_interp) */
  float mb_k[DIG_ABI_MB_MAX * DIG_ABI_MB_MAX]; /* motion-blur kernel of the run, row-major mb_size x mb_size (the rest 0) */
  int jit_order[4];          /* permutation of the jitter ops 0 brightness, 1 contrast, 2 saturation, 3 hue */
  float jit_factor[4];       /* brightness, contrast, saturation U(0.5, 1.5), hue U(-0.1, 0.1) */
  int hue_shift;             /* trunc(hue 255) mod 256 */
  unsigned noise_key[2];     /* Philox key of the Gaussian noise (the sampler's seed, lo / hi) */
  unsigned noise_step;       /* ... and its step */
  int final_buf;             /* the image the tail reads: 0 the crop, 1 region A, 2 region B of the image's workspace */
  int pad0;
  long long ws_off;          /* byte offset of the image's workspace (regions A, B, R: abiaug.inc) */
  int pad[24];
} dig_abi_params;

#ifdef __cplusplus
static_assert(sizeof(dig_abi_run) == 8 * 4, "dig_abi_run is 8 words");
static_assert(sizeof(dig_abi_params) == DIG_ABI_WORDS * 4, "dig_abi_params is DIG_ABI_WORDS words");
static_assert(__builtin_offsetof(dig_abi_params, ws_off) % 8 == 0, "ws_off is 8-byte aligned");
#endif

#endif /* DIG_AUG_TYPES_H */
