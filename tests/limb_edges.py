"""The signed 8-bit limb decomposition of the matrix-core sweep (csrc/sweep_mfma.hip), written out in Python integers and numpy, shared by
tests/test_sweep_forms_cpu.py, tests/test_gpu_sweep_forms.py and tests/test_gpu_parity.py.  Importable without a GPU and without the oracle.

The model follows the header of sweep_mfma.hip and nothing else:

  database residue a in [0, m)  ->  a'' = a - m where a >= 2^28 - 0x808080, else a;  w = a'' + 0x808080 < 2^28;
                                    s_i = byte_i(w) - 128 (i < 3, signed bytes), u_3 = w >> 24 (4 bits)          a'' = sum_i 256^i s_i
  query residue v in [0, m)     ->  w = v + 0x808080;  t_i = byte_i(w) - 128 (i < 3), t_3 = w >> 24 (0 .. 16)     v   = sum_l 256^l t_l
  one term                          a'' v  =  sum_{i,l} s_i t_l 256^(i+l)  ==  sum_{i,l} s_i t_l T_{i+l}  (mod m),   T_w = 256^w mod m
  K terms                           c_{i,l} = sum_k s_{i,k} t_{l,k} (an int32 on the matrix cores), sum = sum_{i,l} c_{i,l} T_{i+l} (64 bits),
                                    result = (sum + m 2^30) mod m

exact() is the product itself in Python integers, straight from the reference-layout arrays; it shares no code with the model, with the oracle's
vectorised cells or with the kernels.  EDGES / sprinkle() place the residues on which the decomposition can go wrong; extreme_pairs() finds the
operand pairs that drive `sum` furthest from zero."""
import itertools
import operator

import numpy as np

N = 2048
P = 268369921
B = 249561089
MODS = (P, B)
BIAS = 0x808080
WRAP = (1 << 28) - BIAS  # the first database residue stored as a - m; as a query value its top limb is 16.  P > WRAP > B: only prime p wraps
K_MAX = 4096  # terms per sum the kernels admit (sweep_mfma_ok, sweep1_mfma_ok)

# the limb edges: 0, 1, m - 1, m - 2, either side of the wrap point, all-(-128) / all-(+127) limb bytes under the largest top limb of the prime, the
# bias and its complement, single-byte borrows
EDGES = {0: [0, 1, P - 1, P - 2, WRAP - 1, WRAP, WRAP + 1, (15 << 24) - BIAS, (14 << 24) - BIAS + 0xFFFFFF, 0x808080, 0x7F7F7F],
         1: [0, 1, B - 1, B - 2, (14 << 24) - BIAS, (13 << 24) - BIAS + 0xFFFFFF, 0x808080, 0x7F7F7F, 0x800000, 0x7FFFFF, 1 << 27]}
RATE = 0.03


def sprinkle(rng, a, limb_axis, rate=RATE):
    """a[..., limb, z] (limb_axis: where the prime's axis is): replace ~3 % of the residues by edge values of their prime, in place"""
    for limb, mod in ((0, P), (1, B)):
        view = np.moveaxis(a, limb_axis, 0)[limb]
        mask = rng.random(view.shape) < rate
        vals = np.array([v for v in EDGES[limb] if v < mod], dtype=np.uint64)
        view[mask] = vals[rng.integers(0, len(vals), size=int(mask.sum()))]


def is_edge(values, prime):
    """which of the residues (of prime 0 = p, 1 = b) are edge values"""
    return np.isin(np.asarray(values, dtype=np.uint64), np.array([v for v in EDGES[prime] if v < MODS[prime]], dtype=np.uint64))


# ---- the model ----------------------------------------------------------------------------------------------------------------------
class Model:
    """the decomposition; the three switches make the defective variants tests/test_sweep_forms_cpu.py holds the edge set against"""

    def __init__(self, wrap_at_point=True, query_top_bits=5, minus128_as_plus=False):
        self.wrap_at_point, self.query_top_bits, self.minus128_as_plus = wrap_at_point, query_top_bits, minus128_as_plus

    def _bytes(self, w):
        s = np.stack([((w >> (8 * i)) & 0xFF) - 128 for i in range(3)], axis=-1)
        return np.where(s == -128, 128, s) if self.minus128_as_plus else s

    def db_limbs(self, a, m):
        """residues [...] -> limbs [..., 4] (int64): three signed bytes and the 4-bit top"""
        a = np.asarray(a, dtype=np.int64)
        wraps = a >= WRAP if self.wrap_at_point else a > WRAP  # (defective: the wrap point itself keeps a, whose top limb 16 does not fit the nibble)
        w = np.where(wraps, a - m, a) + BIAS
        return np.concatenate([self._bytes(w), ((w >> 24) & 0xF)[..., None]], axis=-1)

    def query_limbs(self, v, m):
        """residues [...] -> limbs [..., 4] (int64): three signed bytes and the top limb 0 .. 16"""
        w = np.asarray(v, dtype=np.int64) + BIAS
        return np.concatenate([self._bytes(w), ((w >> 24) & ((1 << self.query_top_bits) - 1))[..., None]], axis=-1)

    def sums(self, a, v, m):
        """K database and K query residues -> (c [4][4] the limb sums, sum the recombined 64-bit value), as Python integers"""
        s, t = self.db_limbs(a, m), self.query_limbs(v, m)
        c = (s.T @ t).tolist()  # |c| <= K 2^14: exact in int64
        return c, sum(c[i][l] * pow(256, i + l, m) for i in range(4) for l in range(4))

    def dot(self, a, v, m):
        """the kernel's result for one output: (sum + m 2^30) mod m"""
        return (self.sums(a, v, m)[1] + (m << 30)) % m


TRUE = Model()
DEFECTS = {"no wrap at 2^28 - 0x808080": Model(wrap_at_point=False), "query top limb cut to 4 bits": Model(query_top_bits=4),
           "byte -128 read as +128": Model(minus128_as_plus=True)}


def recompose(limbs):
    """sum_i 256^i limb_i: a'' of database limbs, v of query limbs"""
    return sum(limbs[..., i] << (8 * i) for i in range(4))


def term_form(s, t, m):
    """sum_{i,l} s_i t_l T_{i+l} of one term's limbs (Python integers)"""
    return sum(int(s[i]) * int(t[l]) * pow(256, i + l, m) for i in range(4) for l in range(4))


def box_bound(m):
    """no term's form exceeds this in magnitude, whatever the residues: every limb at the far end of its box (|byte| <= 128, tops <= 15 and 16)"""
    smax, tmax = (128, 128, 128, 15), (128, 128, 128, 16)
    return sum(smax[i] * tmax[l] * pow(256, i + l, m) for i in range(4) for l in range(4))


def extreme_pairs(m):
    """((database residue, query residue) maximising the per-term form, its value), (the minimising pair, its value).  The form is bilinear in the two
    limb vectors with positive T, so its extremes over the limb boxes are at vertices: every byte limb at -128 or +127, and -- the top limbs are tied
    to the residue range -- every top limb value, kept where the limbs spell a residue below m (for the database: in its stored form)."""
    def candidates(limbs_of, tops):
        out = []
        for by in itertools.product((0x00, 0xFF), repeat=3):
            for top in tops:
                w = by[0] | (by[1] << 8) | (by[2] << 16) | (top << 24)
                x = w - BIAS  # a'' or v
                r = x + m if x < 0 else x
                if 0 <= r < m and int(recompose(limbs_of(np.array([r]), m))[0]) == x:
                    out.append((r, [int(y) for y in limbs_of(np.array([r]), m)[0]]))
        return out

    dbs, qs = candidates(TRUE.db_limbs, range(16)), candidates(TRUE.query_limbs, range(17))
    scored = [(term_form(s, t, m), a, v) for a, s in dbs for v, t in qs]
    hi, lo = max(scored), min(scored)
    return ((hi[1], hi[2]), hi[0]), ((lo[1], lo[2]), lo[0])


# ---- the reference: the product itself ------------------------------------------------------------------------------------------------
def operands(db, query, pos):
    """the K database and K query residues (numpy uint64) that meet in one output word.
    base (query [N][dim0][2][4], reorientCiphertexts; db [N][num_per][2][dim0][2], load_db):  pos = (i, r, c, prime, z) of out [num_per][3][2][2][N]
    pack (query [N][dim0][2], reorientCiphertextsDim1; db [N][num_per][dim0], convertDb):    pos = (i, r, prime, z)    of out [num_per][2][2][N]"""
    query = np.asarray(query)
    dim0 = query.shape[1]
    if query.shape[-1] == 4:
        i, r, c, prime, z = pos
        d = np.asarray(db).reshape(N, -1, 2, dim0, 2)[z, i, c].reshape(-1)
        q = query[z, :, :, r].reshape(-1)
    else:
        i, r, prime, z = pos
        d = np.asarray(db).reshape(N, -1, dim0)[z, i]
        q = query[z, :, r]
    sh, mask = np.uint64(32 * prime), np.uint64(0xFFFFFFFF)
    return (d >> sh) & mask, (q >> sh) & mask


def exact(db, query, positions):
    """the outputs at `positions` (see operands) in Python integers: sum of products, one remainder"""
    out = []
    for pos in positions:
        d, q = operands(db, query, pos)
        out.append(sum(map(operator.mul, d.tolist(), q.tolist())) % MODS[pos[-2]])
    return out


def sample_positions(rng, out_shape, count):
    """`count` positions of an output array [..., prime, z], both primes and the first and last slot among them"""
    pos = [tuple(int(rng.integers(0, n)) for n in out_shape) for _ in range(count)]
    pos[0] = (0,) * len(out_shape)
    pos[1] = tuple(n - 1 for n in out_shape)
    return pos
