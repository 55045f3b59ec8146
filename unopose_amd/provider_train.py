"""MegaPose training-pair provider for the one-reference setting: the producer side of the TRAINING step's input dict
(BASELINE configs[3]).

Contract = the items of ``DatasetPoseFreeOneRefv2`` (core/unopose/provider/pfoneref_training_dataset_v2.py:75-590): the same
directory layout (MegaPose-GSO / MegaPose-ShapeNetCore ``train_pbr_web`` shards, the two "valid instances" and "reference
candidates" json files), the same constructor fields, the same item dict (keys, dtypes, shapes: ``pts``, ``rgb``, ``rgb_choose``,
``translation_label``, ``rotation_label``, ``tem1_rgb``, ``tem1_choose``, ``tem1_pts``, ``K``) and the same consumption of the
global ``np.random`` stream (instance pick, reference pick, colour-augmentation coin, reference point draw, dilation coin,
query point draw, colour-augmentation coin, random rotation, shift, per-point noise), so a seeded epoch reproduces the
reference's samples bit for bit when the colour augmentation is the identity (tests/golden/make_provider_train_golden.py runs the
reference class on the same files).

The structure is this repo's own: one :class:`ViewFiles` value per (shard, key) gives lazily loaded, once-parsed access to the six
files of a MegaPose view; the window / back-projection / resize / normalisation helpers are those of ``provider.py``.

Third-party pieces the reference calls that this image lacks, restated here:
  * ``cv2.dilate(mask, MORPH_CROSS 3x3, iterations=4)`` -> :func:`dilate_cross` (exact: binary dilation by the 4-neighbourhood, four
    times, nothing enters from outside the image; checked against scipy.ndimage.binary_dilation in the tests);
  * ``cv2.resize`` -> ``provider.resize_bilinear_u8`` (see the note there);
  * the imgaug colour-augmentation chain (``aug_code``, :158-176) -> :class:`ColorAugmentor`: the same thirteen operators with the
    same probabilities and parameter ranges, drawn from an own ``np.random.Generator`` (imgaug keeps its own random state too, so the
    global stream is untouched either way).  PARITY UNPINNED for this piece: imgaug is not importable in the build container; the
    operators follow imgaug's documented semantics and the sample statistics are tested, not the pixels."""
import os.path as osp

import numpy as np
import torch

from .provider import Window, lift_depth, load_json, read_image, resize_bilinear_u8, to_tensor_normalize

VIEW_SUFFIXES = (".camera.json", ".depth.png", ".gt_info.json", ".gt.json", ".mask_visib.json", ".rgb.jpg")  # :451-458
SUBSETS = (("GSO", osp.join("MegaPose-GSO", "train_pbr_web"), "megapose_gso_fixed", "gso_models.json"),
           ("ShapeNetCore", osp.join("MegaPose-ShapeNetCore", "train_pbr_web"), "megapose_shapenetcore_fixed", "shapenet_models.json"))


def dilate_cross(mask, iterations=4):
    """cv2.dilate(mask_u8, cv2.getStructuringElement(cv2.MORPH_CROSS, (3, 3)), iterations=n) for a 0/1 mask -> uint8 0/1."""
    m = np.asarray(mask) > 0
    for _ in range(int(iterations)):
        g = m.copy()
        g[1:, :] |= m[:-1, :]
        g[:-1, :] |= m[1:, :]
        g[:, 1:] |= m[:, :-1]
        g[:, :-1] |= m[:, 1:]
        m = g
    return m.astype(np.uint8)


def rle_list_to_mask(rle):
    """MegaPose's mask files hold UNCOMPRESSED COCO run lengths (a list of ints, column-major, starting with a 0-run):
    data_utils.py:168-185."""
    h, w = rle["size"]
    counts = np.asarray(rle["counts"], np.int64)
    runs = np.repeat((np.arange(len(counts)) % 2).astype(bool), counts)[: h * w]
    flat = np.zeros(h * w, dtype=bool)
    flat[: len(runs)] = runs
    return flat.reshape(w, h).T  # column-major, as reshape(h, w, order="F")


def random_rotation_xyz():
    """data_utils.py:286-296: Rx(a0) Ry(a1) Rz(a2) with three angles `np.random.rand(3) * 2 pi` (float64)."""
    a = np.random.rand(3) * 2 * np.pi
    c, s = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    return rx @ ry @ rz


# ---- the colour augmentation as "draw" and "apply" -----------------------------------------------------------------------------------
# Opcodes of an AugPlan entry; csrc/coloraug.hip reads the same numbers (ops/augment.py packs them).
OP_COARSE_DROPOUT, OP_GAUSSIAN_BLUR, OP_SHARPNESS, OP_CONTRAST, OP_BRIGHTNESS, OP_COLOR, OP_ADD = 0, 1, 2, 3, 4, 5, 6
OP_INVERT, OP_MULTIPLY_PC, OP_MULTIPLY, OP_GAUSSIAN_NOISE, OP_LINEAR_CONTRAST, OP_GRAYSCALE = 7, 8, 9, 10, 11, 12
OP_NAMES = ("coarse_dropout", "gaussian_blur", "sharpness", "contrast", "brightness", "color", "add", "invert", "multiply_pc", "multiply",
            "gaussian_noise", "linear_contrast", "grayscale")
BLUR_MIN_SIGMA = 1e-3


class AugPlan:
    """What :meth:`ColorAugmentor.plan` drew for one h x w x 3 image: `ops`, an ordered list of (opcode, params).  params: a float32 scalar
    (blur sigma, the four enhancement factors, grayscale alpha), 3 float32 (add, multiply_pc, multiply, linear_contrast: per channel, a
    shared draw repeated; invert: 1 = flip), the uint8 ch x cw drop grid (1 = drop), or the float32 h x w x 3 noise field."""

    def __init__(self, h=0, w=0, ops=()):
        self.h, self.w, self.ops = int(h), int(w), list(ops)

    def __len__(self):
        return len(self.ops)


def image_to_l(img):
    """Pillow's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    a = img.astype(np.uint32)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def image_blend(deg, img, f):
    """Pillow's Image.blend(deg, img, f) on uint8 arrays with an fp32 factor: t = deg + f (img - deg) in fp32, truncated; clamped to
    0 .. 255 first when f is outside [0, 1]."""
    f = np.float32(f)
    d = deg.astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)
    if not 0 <= f <= 1:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


SMOOTH_KERNEL = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32).reshape(3, 3) / np.float32(13)


def image_smooth(img):
    """Pillow's ImageFilter.SMOOTH ([1 1 1; 1 5 1; 1 1 1] / 13): the border ring is copied (so is an image with a side below 3); inside,
    clamp(floor(0.5 + sum p k)) with the nine products added to 0.5 in row-major order, fp32."""
    out = img.copy()
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return out
    a = img.astype(np.float32)
    s = np.full((h - 2, w - 2) + img.shape[2:], 0.5, np.float32)
    for dy in range(3):
        for dx in range(3):
            s = s + a[dy:dy + h - 2, dx:dx + w - 2] * SMOOTH_KERNEL[dy, dx]
    out[1:-1, 1:-1] = np.clip(np.floor(s), 0, 255).astype(np.uint8)
    return out


def box_blur_weights(sigma, passes=3):
    """Pillow's GaussianBlur(sigma) as `passes` box blurs per axis -> (r, ww, fw): the whole radius, the 8.24 fixed-point weight of a pixel
    inside it and of the two pixels just outside.  fp32, as BoxBlur.c computes it (the square root and the floor in double, rounded once)."""
    f = np.float32
    s2 = f(sigma) * f(sigma) / f(passes)
    L = f(np.sqrt(12.0 * float(s2) + 1.0))
    l = f(np.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * s2)
    a = a / (f(6) * (s2 - (l + f(1)) * (l + f(1))))
    fr = l + a
    r = int(fr)
    ww = int(np.uint32(f(1 << 24) / (fr * f(2) + f(1))))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def _box_line(a, r, ww, fw):
    """One box-blur pass along the last axis of a uint8 array, indices clamped to the line, uint32 wrap-around arithmetic."""
    n = a.shape[-1]
    idx = np.arange(n)
    a32 = a.astype(np.uint32)
    acc = np.zeros(a.shape, np.uint32)
    for k in range(-r, r + 1):
        acc += a32[..., np.clip(idx + k, 0, n - 1)]
    far = a32[..., np.clip(idx - r - 1, 0, n - 1)] + a32[..., np.clip(idx + r + 1, 0, n - 1)]
    return ((acc * np.uint32(ww) + far * np.uint32(fw) + np.uint32(1 << 23)) >> np.uint32(24)).astype(np.uint8)


def image_gaussian_blur(img, sigma, passes=3):
    """Pillow's ImageFilter.GaussianBlur(sigma) on an H x W x C uint8 array: three box passes along the rows, then three along the columns,
    each stored as bytes.  Left alone below BLUR_MIN_SIGMA (ColorAugmentor.gaussian_blur's rule)."""
    if sigma < BLUR_MIN_SIGMA:
        return img
    r, ww, fw = box_blur_weights(sigma, passes)
    x = np.moveaxis(img, 2, 0)  # C, H, W: lines = rows
    for _ in range(passes):
        x = _box_line(x, r, ww, fw)
    x = np.swapaxes(x, 1, 2)  # C, W, H: lines = columns
    for _ in range(passes):
        x = _box_line(x, r, ww, fw)
    return np.ascontiguousarray(np.moveaxis(np.swapaxes(x, 1, 2), 0, 2))


class ColorAugmentor:
    """The reference's colour augmentation (pfoneref_training_dataset_v2.py:158-176; "gdrnpp aug"): thirteen `Sometimes(p, op)`
    applied in a random order per image.  uint8 HxWx3 in, uint8 out.  Own random generator (see the module docstring).

    Two forms: `augment_image` draws and applies in one go (Pillow for the enhancements and the blur); `plan` draws only, consuming the
    generator exactly as `augment_image` would, and `apply` executes a plan in pure numpy.  `apply` is the specification of the device
    route (ops.color_augment) and equals `augment_image` but for grayscale, whose luma it adds elementwise ((R 0.299f + G 0.587f) +
    B 0.114f) where `augment_image` goes through a BLAS product: at most one level apart."""

    def __init__(self, seed=None):
        self.rng = np.random.default_rng(seed)
        self.ops = [(0.5, self.coarse_dropout), (0.4, self.gaussian_blur), (0.3, self.sharpness), (0.3, self.contrast),
                    (0.5, self.brightness), (0.3, self.color), (0.5, self.add), (0.3, self.invert), (0.5, self.multiply_pc),
                    (0.5, self.multiply), (0.1, self.gaussian_noise), (0.5, self.linear_contrast), (0.5, self.grayscale)]

    def augment_image(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.size == 0:
            return img
        for i in self.rng.permutation(len(self.ops)):
            p, op = self.ops[i]
            if self.rng.random() < p:
                img = op(img)
        return img

    __call__ = augment_image

    @staticmethod
    def _u8(x):
        return np.clip(np.rint(x), 0, 255).astype(np.uint8)

    def _enhance(self, img, name, lo, hi):
        from PIL import Image, ImageEnhance

        return np.asarray(getattr(ImageEnhance, name)(Image.fromarray(img)).enhance(float(self.rng.uniform(lo, hi))))

    def coarse_dropout(self, img):  # CoarseDropout(p=0.2, size_percent=0.05): a coarse drop mask, nearest-upsampled, pixels -> 0
        h, w = img.shape[:2]
        ch, cw = max(3, int(round(h * 0.05))), max(3, int(round(w * 0.05)))
        drop = self.rng.random((ch, cw)) < 0.2
        yy = np.minimum((np.arange(h) * ch) // max(h, 1), ch - 1)
        xx = np.minimum((np.arange(w) * cw) // max(w, 1), cw - 1)
        return img * (~drop[yy][:, xx])[:, :, None].astype(np.uint8)

    def gaussian_blur(self, img):  # GaussianBlur(sigma in (0, 3))
        from PIL import Image, ImageFilter

        sigma = float(self.rng.uniform(0.0, 3.0))
        return img if sigma < 1e-3 else np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(sigma)))

    def sharpness(self, img):
        return self._enhance(img, "Sharpness", 0.0, 50.0)

    def contrast(self, img):
        return self._enhance(img, "Contrast", 0.2, 50.0)

    def brightness(self, img):
        return self._enhance(img, "Brightness", 0.1, 6.0)

    def color(self, img):
        return self._enhance(img, "Color", 0.0, 20.0)

    def _per_channel(self, p, draw):
        return draw(3).reshape(1, 1, 3) if self.rng.random() < p else draw(1).reshape(1, 1, 1)

    def add(self, img):  # Add((-25, 25), per_channel=0.3): integer offsets
        return self._u8(img.astype(np.float32) + self._per_channel(0.3, lambda n: self.rng.integers(-25, 26, n).astype(np.float32)))

    def invert(self, img):  # Invert(0.2, per_channel=True)
        flip = self.rng.random(3) < 0.2
        return np.where(flip.reshape(1, 1, 3), 255 - img, img).astype(np.uint8)

    def multiply_pc(self, img):  # Multiply((0.6, 1.4), per_channel=0.5)
        return self._u8(img.astype(np.float32) * self._per_channel(0.5, lambda n: self.rng.uniform(0.6, 1.4, n).astype(np.float32)))

    def multiply(self, img):
        return self._u8(img.astype(np.float32) * np.float32(self.rng.uniform(0.6, 1.4)))

    def gaussian_noise(self, img):  # AdditiveGaussianNoise(scale=10, per_channel=True)
        return self._u8(img.astype(np.float32) + self.rng.normal(0.0, 10.0, img.shape).astype(np.float32))

    def linear_contrast(self, img):  # LinearContrast((0.5, 2.2), per_channel=0.3): 128 + alpha (v - 128)
        a = self._per_channel(0.3, lambda n: self.rng.uniform(0.5, 2.2, n).astype(np.float32))
        return self._u8(128.0 + a * (img.astype(np.float32) - 128.0))

    def grayscale(self, img):  # Grayscale(alpha in (0, 1)): blend with the luma image
        alpha = np.float32(self.rng.uniform(0.0, 1.0))
        g = img.astype(np.float32) @ np.array([0.299, 0.587, 0.114], np.float32)
        return self._u8((1 - alpha) * img.astype(np.float32) + alpha * g[:, :, None])

    # -- draw: one method per operator, the same generator calls in the same order as the operator above
    def _plan_channels(self, p, draw):
        v = draw(3) if self.rng.random() < p else np.repeat(draw(1), 3)
        return v.astype(np.float32)

    def _plan_coarse_dropout(self, h, w):
        ch, cw = max(3, int(round(h * 0.05))), max(3, int(round(w * 0.05)))
        return (self.rng.random((ch, cw)) < 0.2).astype(np.uint8)

    def _plan_gaussian_blur(self, h, w):
        sigma = float(self.rng.uniform(0.0, 3.0))
        return None if sigma < BLUR_MIN_SIGMA else np.float32(sigma)  # None: drawn, but the operator leaves the image alone

    def _plan_sharpness(self, h, w):
        return np.float32(float(self.rng.uniform(0.0, 50.0)))

    def _plan_contrast(self, h, w):
        return np.float32(float(self.rng.uniform(0.2, 50.0)))

    def _plan_brightness(self, h, w):
        return np.float32(float(self.rng.uniform(0.1, 6.0)))

    def _plan_color(self, h, w):
        return np.float32(float(self.rng.uniform(0.0, 20.0)))

    def _plan_add(self, h, w):
        return self._plan_channels(0.3, lambda n: self.rng.integers(-25, 26, n))

    def _plan_invert(self, h, w):
        return (self.rng.random(3) < 0.2).astype(np.float32)

    def _plan_multiply_pc(self, h, w):
        return self._plan_channels(0.5, lambda n: self.rng.uniform(0.6, 1.4, n))

    def _plan_multiply(self, h, w):
        return np.repeat(np.float32(self.rng.uniform(0.6, 1.4)), 3)

    def _plan_gaussian_noise(self, h, w):
        return self.rng.normal(0.0, 10.0, (h, w, 3)).astype(np.float32)

    def _plan_linear_contrast(self, h, w):
        return self._plan_channels(0.3, lambda n: self.rng.uniform(0.5, 2.2, n))

    def _plan_grayscale(self, h, w):
        return np.float32(self.rng.uniform(0.0, 1.0))

    def plan(self, h, w):
        """The draws of `augment_image` for an h x w x 3 image, without the image: the permutation, the coins, every chosen operator's
        parameters, the drop grid and the noise field.  Leaves `self.rng` where `augment_image` would."""
        h, w = int(h), int(w)
        ops = []
        if h * w == 0:
            return AugPlan(h, w)
        for i in self.rng.permutation(len(self.ops)):
            p, op = self.ops[i]
            if self.rng.random() < p:
                name = op.__name__
                params = getattr(self, "_plan_" + name)(h, w)
                if params is not None:
                    ops.append((OP_NAMES.index(name), params))
        return AugPlan(h, w, ops)

    @staticmethod
    def apply_op(img, opcode, params):
        """One plan entry on a uint8 H x W x 3 image, in numpy: integer and fp32 arithmetic exactly as the device kernels do it."""
        u8 = ColorAugmentor._u8
        x = img.astype(np.float32)
        if opcode == OP_COARSE_DROPOUT:
            h, w = img.shape[:2]
            ch, cw = params.shape
            yy = np.minimum((np.arange(h) * ch) // max(h, 1), ch - 1)
            xx = np.minimum((np.arange(w) * cw) // max(w, 1), cw - 1)
            return img * (params[yy][:, xx] == 0)[:, :, None].astype(np.uint8)
        if opcode == OP_GAUSSIAN_BLUR:
            return image_gaussian_blur(img, params)
        if opcode == OP_SHARPNESS:
            return image_blend(image_smooth(img), img, params)
        if opcode == OP_CONTRAST:
            lum = image_to_l(img)
            n = lum.size
            m = (2 * int(lum.sum(dtype=np.int64)) + n) // (2 * n)  # int(mean + 0.5)
            return image_blend(np.full_like(img, m), img, params)
        if opcode == OP_BRIGHTNESS:
            return image_blend(np.zeros_like(img), img, params)
        if opcode == OP_COLOR:
            return image_blend(np.repeat(image_to_l(img)[:, :, None], 3, axis=2), img, params)
        if opcode in (OP_ADD, OP_GAUSSIAN_NOISE):
            return u8(x + (params if opcode == OP_GAUSSIAN_NOISE else params.reshape(1, 1, 3)))
        if opcode == OP_INVERT:
            return np.where(params.reshape(1, 1, 3) != 0, 255 - img, img).astype(np.uint8)
        if opcode in (OP_MULTIPLY_PC, OP_MULTIPLY):
            return u8(x * params.reshape(1, 1, 3))
        if opcode == OP_LINEAR_CONTRAST:
            return u8(np.float32(128.0) + params.reshape(1, 1, 3) * (x - np.float32(128.0)))
        if opcode == OP_GRAYSCALE:
            alpha = np.float32(params)
            g = (x[..., 0] * np.float32(0.299) + x[..., 1] * np.float32(0.587)) + x[..., 2] * np.float32(0.114)
            return u8((np.float32(1) - alpha) * x + alpha * g[:, :, None])
        raise ValueError(f"ColorAugmentor.apply: opcode {opcode}")

    def apply(self, img, plan):
        """`plan` on `img` (uint8 H x W x 3) -> uint8.  Pure numpy, no Pillow, no generator."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.size == 0 or len(plan) == 0:
            return img
        if img.shape != (plan.h, plan.w, 3):
            raise ValueError(f"ColorAugmentor.apply: image {img.shape} for a plan over {plan.h} x {plan.w}")
        for opcode, params in plan.ops:
            img = np.ascontiguousarray(self.apply_op(img, opcode, params))
        return img


class ViewFiles:
    """The six files of one MegaPose view ``<root>/<subset>/<shard:06d>/<key>.*``, each parsed at most once."""

    def __init__(self, head):
        self.head = head
        self._camera = self._gt = self._masks = None

    def complete(self):
        return all(osp.exists(self.head + s) for s in VIEW_SUFFIXES)

    @property
    def camera(self):
        if self._camera is None:
            self._camera = load_json(self.head + ".camera.json")
        return self._camera

    @property
    def K(self):
        return np.array(self.camera["cam_K"]).reshape(3, 3).astype(np.float32)

    def pose(self, inst):
        """4 x 4 float32 object-to-camera pose of instance `inst` (translation in metres) and its obj_id."""
        if self._gt is None:
            self._gt = load_json(self.head + ".gt.json")
        g = self._gt[inst]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.array(g["cam_R_m2c"], np.float32).reshape(3, 3)
        T[:3, 3] = np.array(g["cam_t_m2c"], np.float32).reshape(3) / 1000.0
        return T, g["obj_id"]

    def mask(self, inst_id=None, position=None):
        """Visible mask (bool H x W) of the instance with id `inst_id`, or of the `position`-th instance in id order (the
        reference indexes the stacked, id-sorted masks with the valid-instance number: :247)."""
        if self._masks is None:
            self._masks = {int(k): v for k, v in load_json(self.head + ".mask_visib.json").items()}
        if inst_id is None:
            inst_id = sorted(self._masks)[position]
        return rle_list_to_mask(self._masks[inst_id])

    def depth_m(self):
        return read_image(self.head + ".depth.png").astype(np.float32) * self.camera["depth_scale"] / 1000.0

    def colour(self):
        return read_image(self.head + ".rgb.jpg").astype(np.uint8)


class MegaPoseOneRefTrainSet:
    """cfg: data_dir, img_size, n_sample_observed_point, n_sample_model_point, n_sample_template_point, min_px_count_visib,
    min_visib_fract, dilate_mask, rgb_mask_flag, shift_range, optional rgb_to_bgr (attribute or key access).
    ``color_augmentor``: "default" -> :class:`ColorAugmentor`; None -> identity; or any object with ``augment_image``.
    Usage as the reference's (build_data_loader.py): ``ds.reset()`` once per epoch, then ``ds[i]`` for i < len(ds).
    ``device_crops=True``: an item carries, in place of ``rgb`` and ``tem1_rgb``, the unfinished crop of each image -- ``rgb_crop`` (uint8
    window crop, after the BGR option), ``rgb_cropmask`` (uint8 0 / 1), ``rgb_plan`` (the :class:`AugPlan` drawn for it; empty where the
    0.8 coin failed or there is no augmentor) and the ``tem1_*`` equivalents -- for :func:`collate_pairs_device` and ``ops.finish_crops``.
    Every draw from ``np.random`` and from the augmentor's generator happens at the same point on both routes; the augmentor must have
    ``plan``."""

    def __init__(self, cfg, num_img_per_epoch=-1, color_augmentor="default", seed=None, device_crops=False):
        get = (lambda k, *d: cfg.get(k, *d)) if hasattr(cfg, "get") else (lambda k, *d: getattr(cfg, k, *d))
        self.device_crops = bool(device_crops)
        self.data_dir = get("data_dir")
        self.num_img_per_epoch = num_img_per_epoch
        self.dilate_mask, self.rgb_mask_flag = get("dilate_mask"), get("rgb_mask_flag")
        self.shift_range, self.img_size = get("shift_range"), get("img_size")
        self.n_obs, self.n_tpl = get("n_sample_observed_point"), get("n_sample_template_point")
        self.bgr = get("rgb_to_bgr", False)
        self.views, self.subset_dir, self.references, self.valid = [], {}, {}, {}
        for name, rel, prefix, _models in SUBSETS:
            self.subset_dir[name] = rel
            shards = load_json(osp.join(self.data_dir, rel, "key_to_shard.json"))
            self.views += [(name, f"{shards[k]:06d}", k) for k in shards]  # key order of the json file (:119-124)
            self.references[name] = load_json(osp.join(self.data_dir, prefix + "_obj_id_to_visib0_8_scene_im_inst_ids.json"))
            self.valid[name] = load_json(osp.join(self.data_dir, prefix + "_valid_inst_ids.json"))
        self.length = len(self.views)
        self.color_augmentor = ColorAugmentor(seed) if isinstance(color_augmentor, str) else color_augmentor
        self.img_idx = None

    def __len__(self):
        return self.length if self.num_img_per_epoch == -1 else self.num_img_per_epoch

    def reset(self):
        """Draw the epoch's view indices (:182-191)."""
        if self.num_img_per_epoch == -1:
            self.num_img_per_epoch = self.length
        self.img_idx = np.random.choice(self.length, self.num_img_per_epoch, replace=self.length <= self.num_img_per_epoch)

    def __getitem__(self, index):
        while True:  # a view without a usable sample is replaced by another position of the epoch (:193-204)
            item = self.read_data(self.img_idx[index])
            if item is not None:
                return item
            index = np.random.choice([i for i in range(len(self)) if i != index])

    def _files(self, subset, shard, key):
        return ViewFiles(osp.join(self.data_dir, self.subset_dir[subset], shard, key))

    def _crop_tensor(self, files, win, mask):
        """colour -> window -> (80 %: colour augmentation) -> foreground only -> resize -> ImageNet-normalised CHW."""
        rgb = files.colour()
        rgb = win.crop(rgb[..., ::-1] if self.bgr else rgb)
        if self.device_crops:  # the same coin and generator draws; the pixels are left to ops.finish_crops
            plan = AugPlan()
            if np.random.rand() < 0.8 and self.color_augmentor is not None:
                plan = self.color_augmentor.plan(rgb.shape[0], rgb.shape[1])
            return np.ascontiguousarray(rgb, dtype=np.uint8), np.ascontiguousarray(mask > 0).view(np.uint8), plan
        if np.random.rand() < 0.8 and self.color_augmentor is not None:
            rgb = self.color_augmentor.augment_image(rgb)
        if self.rgb_mask_flag:
            rgb = rgb * (mask[:, :, None] > 0).astype(np.uint8)
        return to_tensor_normalize(resize_bilinear_u8(np.ascontiguousarray(rgb), self.img_size))

    @staticmethod
    def _draw(n_have, n_want):
        return np.random.choice(np.arange(n_have), n_want, replace=n_have <= n_want)

    def reference_view(self, subset, obj_id):
        """One random reference view of the object (:399-449) -> (rgb CHW, choose (n_tpl,), camera-space points (n_tpl,3) float64,
        4 x 4 pose) or None."""
        cands = self.references[subset][str(obj_id)]
        if len(cands) == 0:
            return None
        shard, key, inst = cands[np.random.choice(list(range(len(cands))))]
        files = self._files(subset, f"{shard:06d}", key)
        mask = files.mask(inst_id=inst)
        if mask.sum() == 0:
            return None
        win = Window.around(mask)
        mask = win.crop(mask)
        if mask.sum() == 0:
            return None
        rgb = self._crop_tensor(files, win, mask)
        choose = mask.astype(np.float32).flatten().nonzero()[0]
        choose = choose[self._draw(len(choose), self.n_tpl)]
        K = files.K
        xyz = lift_depth(files.depth_m(), K, win).reshape(-1, 3)[choose]
        return rgb, win.to_resized(choose, self.img_size), xyz, files.pose(inst)[0]

    def read_data(self, index):
        subset, shard, key = self.views[index]
        files = self._files(subset, shard, key)
        if not files.complete():
            return None
        insts = self.valid[subset].get(f"{shard}/{key}", [])
        if len(insts) == 0:
            return None
        inst = insts[np.random.randint(0, len(insts))]  # one valid instance per visit (:208-210)
        pose_q, obj_id = files.pose(inst)
        assert len(self.references[subset][str(obj_id)]) != 0
        K = files.K
        ref = self.reference_view(subset, obj_id)
        if ref is None:
            return None
        tem_rgb, tem_choose, tem_pts, pose_r = ref
        rel = pose_q @ np.linalg.inv(pose_r)  # reference camera -> query camera (float32, :242)
        radius = np.max(np.linalg.norm(tem_pts - np.mean(tem_pts, axis=0).reshape(1, 3), axis=1))

        mask = files.mask(position=inst)
        if np.sum(mask) == 0:
            return None
        if self.dilate_mask and np.random.rand() < 0.5:
            mask = dilate_cross(mask, 4)
        win = Window.around(mask > 0)
        mask = win.crop(mask)
        if np.sum(mask) == 0:
            return None
        choose = mask.astype(np.float32).flatten().nonzero()[0]
        pts = lift_depth(files.depth_m(), K, win).reshape(-1, 3)[choose]
        keep = np.linalg.norm(pts - np.mean(pts, axis=0).reshape(1, 3), axis=1) < 1.2 * radius  # outliers w.r.t. the reference's extent
        pts, choose = pts[keep], choose[keep]
        if len(choose) < 32:
            return None
        sel = self._draw(len(choose), self.n_obs)
        choose, pts = choose[sel], pts[sel]
        rgb = self._crop_tensor(files, win, mask)
        rgb_choose = win.to_resized(choose, self.img_size)

        # rotation augmentation of the reference cloud, translation shift + per-point noise on the query cloud (:336-356)
        spin = np.eye(4, dtype=np.float32)
        spin[:3, :3] = random_rotation_xyz()
        tem_pts = tem_pts @ spin[:3, :3]
        target = rel @ spin
        shift = np.random.uniform(-self.shift_range, self.shift_range, (1, 3))
        target_t = target[:3, 3] + shift[0]
        pts = np.add(pts, shift + 0.001 * np.random.randn(pts.shape[0], 3))
        item = {"pts": torch.FloatTensor(pts), "rgb": None, "rgb_choose": torch.IntTensor(rgb_choose).long(),
                "translation_label": torch.FloatTensor(target_t), "rotation_label": torch.FloatTensor(target[:3, :3]),
                "tem1_rgb": None, "tem1_choose": torch.IntTensor(tem_choose).long(),
                "tem1_pts": torch.FloatTensor(tem_pts), "K": torch.FloatTensor(K)}
        for key, stem, image in (("rgb", "rgb_", rgb), ("tem1_rgb", "tem1_", tem_rgb)):
            if self.device_crops:  # (uint8 crop, uint8 crop mask, AugPlan) in place of the finished tensor
                del item[key]
                item.update(zip((stem + "crop", stem + "cropmask", stem + "plan"), image))
            else:
                item[key] = torch.FloatTensor(image)
        return item


def collate_pairs(items):
    """Default collation of the training loader: stack every key (all items have the same shapes)."""
    return {k: torch.stack([it[k] for it in items]) for k in items[0]}


# ---- the device route: crops, masks and plans travel to the training process, ops.finish_crops finishes them there -------------------
AUG_DESC_INTS, AUG_ENTRY_INTS = 8, 4  # csrc/coloraug.hip's CAUG_DESC / CAUG_ENTRY (ops.color_augment checks they agree)
CROP_KEYS = ("crop_atlas", "crop_desc", "crop_ops", "crop_grids", "crop_noise", "crop_masks", "crop_rows", "crop_cfg")


def _bits(values):
    return np.asarray(values, dtype=np.float32).reshape(-1).view(np.int32)


def pack_plans(boxes, plans):
    """The tables csrc/coloraug.hip reads, on the host: boxes = one (y0, h, w) per crop (its rows in the atlas), plans = one AugPlan (or
    None = empty) per crop -> (desc (n, 8) int32, ops (entries, 4) int32, grids uint8, noise float32), laid out as the kernel file
    documents.  Never empty arrays: unused tables hold one element."""
    desc = np.zeros((len(boxes), AUG_DESC_INTS), np.int64)
    entries, grids, noise = [], [], []
    n_grid = n_noise = n_sums = 0
    for c, ((y0, h, w), plan) in enumerate(zip(boxes, plans)):
        ops = [] if plan is None else plan.ops
        if ops and (plan.h, plan.w) != (h, w):
            raise ValueError(f"pack_plans: a plan over {plan.h} x {plan.w} for a {h} x {w} crop")
        desc[c, :7] = (y0, h, w, len(ops), len(entries), n_grid, n_noise)
        g_rel = z_rel = 0
        for opcode, params in ops:
            e = np.zeros(AUG_ENTRY_INTS, np.int32)
            e[0] = opcode
            if opcode == OP_COARSE_DROPOUT:
                grid = np.ascontiguousarray(params, dtype=np.uint8)
                e[1:4] = (grid.shape[0], grid.shape[1], g_rel)
                grids.append(grid.reshape(-1))
                g_rel += grid.size
            elif opcode == OP_GAUSSIAN_BLUR:
                r, ww, fw = box_blur_weights(params)
                e[1:4] = np.array([r, ww, fw], np.uint32).view(np.int32)
            elif opcode == OP_GAUSSIAN_NOISE:
                field = np.ascontiguousarray(params, dtype=np.float32)
                if field.shape != (h, w, 3):
                    raise ValueError(f"pack_plans: noise {field.shape} for a {h} x {w} crop")
                e[1] = z_rel
                noise.append(field.reshape(-1))
                z_rel += field.size
            elif opcode == OP_CONTRAST:
                e[1], e[2] = _bits(params)[0], n_sums
                n_sums += 1
            elif opcode in (OP_SHARPNESS, OP_BRIGHTNESS, OP_COLOR, OP_GRAYSCALE):
                e[1] = _bits(params)[0]
            elif opcode in (OP_ADD, OP_INVERT, OP_MULTIPLY_PC, OP_MULTIPLY, OP_LINEAR_CONTRAST):
                e[1:4] = _bits(params)
            else:
                raise ValueError(f"pack_plans: opcode {opcode}")
            entries.append(e)
        n_grid, n_noise = n_grid + g_rel, n_noise + z_rel
    if max(n_noise, n_grid, int(desc.max(initial=0))) >= 2 ** 31:
        raise ValueError("pack_plans: too many values for 32-bit offsets")
    return (desc.astype(np.int32), np.stack(entries) if entries else np.zeros((1, AUG_ENTRY_INTS), np.int32),
            np.concatenate(grids) if grids else np.zeros(1, np.uint8), np.concatenate(noise) if noise else np.zeros(1, np.float32))


def build_atlas(crops):
    """uint8 h x w x 3 crops one under the other -> (atlas (sum h, max w, 3) uint8, rows right of a crop's width zero; boxes (y0, h, w))."""
    boxes, y = [], 0
    for c in crops:
        boxes.append((y, c.shape[0], c.shape[1]))
        y += c.shape[0]
    atlas = np.zeros((y, max(c.shape[1] for c in crops), 3), np.uint8)
    for (y0, h, w), c in zip(boxes, crops):
        atlas[y0:y0 + h, :w] = c
    return atlas, boxes


def collate_pairs_device(items, img_size, rgb_mask_flag=True):
    """Collation of `device_crops=True` items: the B query crops, then the B reference crops, in one atlas with their descriptors, plan
    tables, packed window masks and per-row mask counts (what `ops.finish_crops` uploads and finishes); every other key stacked."""
    images = [(it[p + "_crop"], it[p + "_cropmask"], it[p + "_plan"]) for p in ("rgb", "tem1") for it in items]
    crops = [np.asarray(im[0]) for im in images]
    atlas, boxes = build_atlas(crops)
    desc, ops, grids, noise = pack_plans(boxes, [im[2] for im in images])
    masks = [np.ascontiguousarray(np.asarray(im[1]) != 0) for im in images]
    for m, (_, h, w) in zip(masks, boxes):
        if m.shape != (h, w):
            raise ValueError(f"collate_pairs_device: mask {m.shape} for a {h} x {w} crop")
    skip = {f"{p}_{s}" for p in ("rgb", "tem1") for s in ("crop", "cropmask", "plan")}
    batch = {k: torch.stack([it[k] for it in items]) for k in items[0] if k not in skip}
    batch.update(crop_atlas=torch.from_numpy(atlas), crop_desc=torch.from_numpy(desc), crop_ops=torch.from_numpy(ops),
                 crop_grids=torch.from_numpy(grids), crop_noise=torch.from_numpy(noise),
                 crop_masks=torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks]).view(np.uint8)),
                 crop_rows=torch.from_numpy(np.concatenate([m.sum(axis=1, dtype=np.int64) for m in masks]).astype(np.int32)),
                 crop_cfg=torch.tensor([int(img_size), int(bool(rgb_mask_flag))], dtype=torch.int32))
    return batch
