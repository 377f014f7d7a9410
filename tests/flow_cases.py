"""Seeded inputs of the flow tests: band-limited noise textures (white noise shaped by a Gaussian spectrum of `sigma`
cycles / px, quantised to uint8), a second image cut from the same larger texture at an integer offset (optionally with added
noise), and the point sets.  Built once per process and shared (callers do not write into them)."""
import functools

import numpy as np

import flow_oracle as fo

WIN = (15, 15)
MARGIN = 16                      # the larger texture extends this far beyond the first image on every side
PLANTED_SHIFTS = [(3, -2), (9, 6), (-5, 4)]
PLANTED_SIZES = [(96, 128), (61, 75)]          # (H, W)


def texture(H, W, sigma, seed):
    """uint8 [H][W]: white noise through a Gaussian spectrum of `sigma` cycles / px, mean 128, standard deviation 48."""
    rs = np.random.RandomState(seed)
    white = rs.standard_normal((H, W))
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    shaped = np.fft.ifft2(np.fft.fft2(white) * np.exp(-(fx * fx + fy * fy) / (2.0 * sigma * sigma))).real
    shaped = (shaped - shaped.mean()) / shaped.std()
    return np.clip(np.rint(128.0 + 48.0 * shaped), 0, 255).astype(np.uint8)


def image_pair(H, W, shift, sigma=0.08, seed=0, noise_sd=0.0):
    """(first, second): second(x, y) = first(x - dx, y - dy), i.e. a feature at p in the first image is at p + shift in the
    second; both are windows of one (H + 2 MARGIN) x (W + 2 MARGIN) texture."""
    dx, dy = shift
    assert abs(dx) <= MARGIN and abs(dy) <= MARGIN
    big = texture(H + 2 * MARGIN, W + 2 * MARGIN, sigma, seed)
    first = big[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    second = big[MARGIN - dy:MARGIN - dy + H, MARGIN - dx:MARGIN - dx + W]
    if noise_sd > 0:
        rs = np.random.RandomState(seed + 7919)
        second = np.clip(np.rint(second + noise_sd * rs.standard_normal(second.shape)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(first), np.ascontiguousarray(second)


def interior_points(H, W, n, inset, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(inset, W - 1 - inset, n), rs.uniform(inset, H - 1 - inset, n)], axis=1).astype(np.float32)


class Case:
    """One tracking problem and its oracle result (computed on first use)."""

    def __init__(self, name, first, second, pts, init=None, win=WIN, max_level=2, max_iter=10, eps=0.03, planted=None):
        self.name, self.first, self.second, self.pts, self.init = name, first, second, pts, init
        self.win, self.max_level, self.max_iter, self.eps, self.planted = win, max_level, max_iter, eps, planted
        H, W = first.shape
        self.levels = fo.pyramid_levels(H, W, win, max_level)
        self._result = None

    @property
    def pyramids(self):
        if getattr(self, "_pyr", None) is None:
            self._pyr = fo.Pyramid(self.first, self.levels), fo.Pyramid(self.second, self.levels)
        return self._pyr

    @property
    def result(self):
        """(next, status, matches0, trace, margins) of the oracle."""
        if self._result is None:
            pi, pj = self.pyramids
            self._result = fo.track(pi, pj, self.pts, self.init, self.win, self.max_iter, self.eps)
        return self._result


@functools.lru_cache(maxsize=None)
def planted_cases():
    """(b): planted integer shifts, 40 points at least 20 px inside."""
    out = []
    for k, (H, W) in enumerate(PLANTED_SIZES):
        for s, shift in enumerate(PLANTED_SHIFTS):
            a, b = image_pair(H, W, shift, sigma=0.08, seed=10 * k + s)
            out.append(Case(f"planted_{H}x{W}_{shift[0]}_{shift[1]}", a, b, interior_points(H, W, 40, 20, 100 + 10 * k + s),
                            planted=shift))
    return out


@functools.lru_cache(maxsize=None)
def constant_case():
    """(c): nothing to track."""
    img = np.full((48, 64), 93, np.uint8)
    return Case("constant", img, img.copy(), interior_points(48, 64, 9, 5, 3))


@functools.lru_cache(maxsize=None)
def short_pyramid_case():
    """(d): 48 x 64 with max_level 3 stops at L = 1 (level 2 would be 12 high, not above the 15-px window)."""
    a, b = image_pair(48, 64, (2, 1), sigma=0.1, seed=21)
    return Case("short_pyramid", a, b, interior_points(48, 64, 12, 10, 22), max_level=3, planted=(2, 1))


@functools.lru_cache(maxsize=None)
def border_case():
    """(e): corner points and a fractional point near the edge under a 1-px shift; (-20, 5) cannot be tracked."""
    H, W = 64, 80
    a, b = image_pair(H, W, (1, 0), sigma=0.08, seed=31)
    pts = np.array([[0, 0], [W - 1, H - 1], [1.25, H - 2.5], [-20, 5]], np.float32)
    return Case("border", a, b, pts, planted=(1, 0))


NOISY_SEED = 1          # picked on the CPU: the first seed whose trace holds every iteration count and exit code test (f) asks for


@functools.lru_cache(maxsize=None)
def noisy_case():
    """(f): 96 x 128, noise sd 12, sigma 0.1, 200 points from [-5, W + 5] x [-5, H + 5].  A point of that range cannot fail the
    first range test at level 0 (that needs x < -8 or x >= W + 7 with a 15-px window), so two points beyond it are appended for
    exit code 5: 202 points."""
    H, W = 96, 128
    a, b = image_pair(H, W, (4, -3), sigma=0.1, seed=NOISY_SEED, noise_sd=12.0)
    rs = np.random.RandomState(1000 + NOISY_SEED)
    pts = np.stack([rs.uniform(-5, W + 5, 200), rs.uniform(-5, H + 5, 200)], axis=1).astype(np.float32)
    pts = np.concatenate([pts, np.array([[-20, 5], [W + 9.5, H / 2]], np.float32)])
    return Case("noisy", a, b, pts)


@functools.lru_cache(maxsize=None)
def guess_case():
    """The (9, 6) planted pair with an initial guess up to 1.5 px off the planted position on each axis."""
    base = planted_cases()[1]
    rs = np.random.RandomState(77)
    init = (base.pts + np.array(base.planted, np.float32) + rs.uniform(-1.5, 1.5, base.pts.shape)).astype(np.float32)
    return Case("guess", base.first, base.second, base.pts, init=init, planted=base.planted)


def all_cases():
    return planted_cases() + [constant_case(), short_pyramid_case(), border_case(), noisy_case(), guess_case()]
