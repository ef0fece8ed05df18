"""Host-side initial images of drawers.Raw (perceptor/drawers/raw/init/{fractal,gradient}.py), numpy float64 -> torch fp32.

Both draw from the global ``np.random`` state in the reference's order, so a seeded call reproduces the reference's picture:
fractal: per sample, per channel, per octave one ``rand(res + 1, res + 1)`` lattice of gradient angles; gradient: per sample
``randint(0, 255)``, ``randint(1, 255)``, ``randint(2, 255)``, ``randint(3, 128)``.
"""
import numpy as np
import torch


def _fade(t):
    return t * t * t * (t * (t * 6 - 15) + 10)          # the quintic 6 t^5 - 15 t^4 + 10 t^3


def _perlin(side: int, res: int) -> np.ndarray:
    """One octave of 2-D Perlin noise on a side x side grid with res x res lattice cells (res divides side)."""
    angle = 2 * np.pi * np.random.rand(res + 1, res + 1)
    gx, gy = np.cos(angle), np.sin(angle)
    cell = side // res
    pos = (np.arange(side) * (res / side)) % 1             # position inside the lattice cell, the same along both axes
    u, v = pos[:, None], pos[None, :]
    i, j = (np.arange(side) // cell)[:, None], (np.arange(side) // cell)[None, :]

    def corner(di, dj):                                     # gradient at the corner . offset from that corner
        return (u - di) * gx[i + di, j + dj] + (v - dj) * gy[i + di, j + dj]

    tu, tv = _fade(u), _fade(v)
    near = corner(0, 0) * (1 - tu) + tu * corner(1, 0)
    far = corner(0, 1) * (1 - tu) + tu * corner(1, 1)
    return np.sqrt(2) * ((1 - tv) * near + tv * far)


def _fractal_plane(side: int, octaves: int) -> np.ndarray:
    total, res, amplitude = np.zeros((side, side)), 32, 1.0
    for _ in range(octaves):
        total += amplitude * _perlin(side, res)
        res *= 2
        amplitude *= 0.5
    n = (total - total.min()) / (total.max() - total.min())
    n = 0.9998 * n + 0.0001                                 # keep the odds finite
    odds = n / (1 - n)
    return 1 / (1 + np.power(odds, -2))                    # the contrast curve odds^2 / (1 + odds^2)


def fractal(shape) -> torch.Tensor:
    """[n, c, h, w] fractal noise in (0, 1): each plane is the top-left h x w crop of a power-of-two square."""
    n, c, h, w = shape
    big = max(h, w)
    side, octaves = (2048, 6) if big > 1024 else (1024, 5) if big > 512 else (512, 4) if big > 256 else (256, 3)
    planes = [[_fractal_plane(side, octaves)[:h, :w] for _ in range(c)] for _ in range(n)]
    return torch.from_numpy(np.asarray(planes)).float()


def gradient(shape) -> torch.Tensor:
    """[n, 3, h, w] colour ramps: red grows left to right from 0, green and blue top to bottom, with random end points."""
    n, c, h, w = shape
    if c != 3:
        raise ValueError("Only 3 channel images are supported.")
    out = np.empty((n, 3, h, w))
    for k in range(n):
        blue0 = np.random.randint(0, 255)
        red1, green1, blue1 = np.random.randint(1, 255), np.random.randint(2, 255), np.random.randint(3, 128)
        out[k, 0] = np.linspace(0, red1, w)[None, :]
        out[k, 1] = np.linspace(0, green1, h)[:, None]
        out[k, 2] = np.linspace(blue0, blue1, h)[:, None]
    return torch.from_numpy(out / 255).float()
