"""The sky, the HDR table and the rotated frame that tests/test_envlight.py and tests/shadow_matrix_cases.py share.  A plain helper
module."""
import numpy as np

F32 = np.float32
# a sun of 18 degrees radius low on the -x side of the canonical camera (which looks down +z)
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.95, sun_color=(30.0, 24.0, 16.0))


def rotation():
    a, b = 0.7, -0.4
    ra = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rb = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (ra @ rb).astype(F32)


def hdr(n):
    """A strongly non-uniform random HDR table, values up to 1e4"""
    return (np.random.default_rng(100 + n).random((n, n, 3)) ** 8 * 1e4).astype(F32)
