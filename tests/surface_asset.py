"""A synthetic ManoAsset that is a real surface with local skinning, for the registration tests.  The project's synthetic
assets (hands_amd.synthetic_mano_asset) have random triangles and random skinning: a triangle soup, on which a distance is
well defined and registration is not -- ICP lowers the cloud's distance there while the vertices stay centimetres off.

``tube_hand_asset``: five capped tubes (fingers: 17 rings of 8 vertices and an apex, 137 vertices each) on a flat 3 x 31 palm
strip: 778 vertices, 1440 faces, the list padded to 1538 with repeats of face 0.  A finger's three joints regress to the
centres of its rings 0, 6 and 11; the skinning weights blend smoothly along the tube (smoothstep over four rings about each
joint), the palm follows the wrist; the ten shape directions are smooth, small sinusoids of the rest position; posedirs is
1e-4 noise.  A round tube does not observe twist about its axis, so tests on it claim distances, not vertices.
"""
import numpy as np

from hands_amd.mano import ManoAsset

RINGS, AROUND, RADIUS, SPACING = 17, 8, 0.008, 0.005
JOINT_RINGS = (0, 6, 11)
PALM_ROWS, PALM_COLS = 3, 31
N_TUBE = RINGS * AROUND + 1


def _smooth(x):
    x = np.clip(x, 0.0, 1.0)
    return x * x * (3.0 - 2.0 * x)


def tube_hand_asset(is_rhand=True):
    rng = np.random.RandomState(7 if is_rhand else 8)
    v, faces, W = [], [], []
    Jreg = np.zeros((16, 778))
    base_x = np.linspace(-0.036, 0.036, 5)
    ang = 2.0 * np.pi * np.arange(AROUND) / AROUND
    for f in range(5):
        o = len(v)
        for r in range(RINGS):
            rad = RADIUS * (1.0 - 0.3 * r / (RINGS - 1))
            for a in ang:
                v.append([base_x[f] + rad * np.cos(a), SPACING * r, rad * np.sin(a)])
            a1, a2, a3 = _smooth((r + 2) / 4.0), _smooth((r - 4) / 4.0), _smooth((r - 9) / 4.0)
            w = np.zeros(16)
            w[0], w[1 + 3 * f], w[2 + 3 * f], w[3 + 3 * f] = 1 - a1, a1 - a2, a2 - a3, a3
            W += [w] * AROUND
        v.append([base_x[f], SPACING * (RINGS - 1) + 0.6 * RADIUS, 0.0])         # the apex
        W.append(W[-1])
        for r in range(RINGS - 1):
            for k in range(AROUND):
                p, q = o + r * AROUND + k, o + r * AROUND + (k + 1) % AROUND
                faces += [[p, p + AROUND, q], [q, p + AROUND, q + AROUND]]
        top = o + (RINGS - 1) * AROUND
        faces += [[top + k, o + N_TUBE - 1, top + (k + 1) % AROUND] for k in range(AROUND)]
        for n, r in enumerate(JOINT_RINGS):
            Jreg[1 + 3 * f + n, o + r * AROUND:o + (r + 1) * AROUND] = 1.0 / AROUND
    o = len(v)
    for r in range(PALM_ROWS):
        for c in range(PALM_COLS):
            v.append([-0.045 + 0.003 * c, -0.012 * (PALM_ROWS - r), 0.0])
            W.append(np.eye(16)[0])
    for r in range(PALM_ROWS - 1):
        for c in range(PALM_COLS - 1):
            p = o + r * PALM_COLS + c
            faces += [[p, p + 1, p + PALM_COLS], [p + 1, p + PALM_COLS + 1, p + PALM_COLS]]
    Jreg[0, o:] = 1.0 / (PALM_ROWS * PALM_COLS)
    v, W, faces = np.array(v), np.array(W), np.array(faces, np.int64)
    assert v.shape == (778, 3) and faces.shape == (1440, 3) and np.allclose(W.sum(1), 1.0)
    faces = np.concatenate([faces, np.repeat(faces[:1], 1538 - len(faces), 0)])
    k = rng.uniform(10.0, 40.0, (10, 3))
    ph = rng.uniform(0.0, 2.0 * np.pi, (10, 3))
    shapedirs = 0.002 * np.sin(np.einsum("nc,lc->nl", v, k)[:, None, :] + ph.T[None])          # (778, 3, 10)
    posedirs = 1e-4 * rng.randn(135, 778 * 3)
    hands_mean = 0.1 * rng.randn(45)
    if not is_rhand:
        v[:, 0], shapedirs[:, 0] = -v[:, 0], -shapedirs[:, 0]
        faces = faces[:, ::-1].copy()
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return ManoAsset(f32(v), f32(shapedirs), f32(posedirs), f32(Jreg), f32(W), f32(hands_mean), faces, is_rhand).validate()
