"""The SpiralPack record layout of include/spiral_gpu.h ("Records", SpiralPack) restated in numpy for the pack record tests.  Nothing here calls the
library under test: the layout is arithmetic on (p_db, nu1, nu2, out_n, S), the splice works on plaintext coefficients, one bit at a time (the bit
helpers are those of tests/records_restated.py).

An item is [trials][2048] coefficients, trials = out_n^2: row t is the item's 1 x 1 plaintext in trial t (output polynomial (t // out_n, t % out_n) of
a decoded response).  Its stream is the little-endian string of w-bit coefficients, trial t's first coefficient at bit t * 2048 * w, i.e. the
concatenation over t of what pack_server_read_db_items(trial = t, w) returns for the item."""
import numpy as np

from records_restated import N, Layout, bits_of, coeffs_of, stream_of  # noqa: F401


def layout(p_db: int, nu1: int, nu2: int, out_n: int, record_bytes: int) -> Layout:
    """None where the layout is refused (more than 16 instances)"""
    w = p_db.bit_length() - 1  # floor(log2 p_db)
    item_bytes = out_n * out_n * 256 * w
    if record_bytes <= item_bytes:
        per_item, instances = item_bytes // record_bytes, 1
    else:
        per_item, instances = 1, -(-record_bytes // item_bytes)
        if instances > 16:
            return None
    return Layout(w, item_bytes, per_item, instances, (1 << (nu1 + nu2)) * per_item)


def place(lay: Layout, record_bytes: int, r: int, instance: int = 0):
    """where instance `instance` keeps record r: (item, byte offset in the item's stream, bytes, first byte of the record they are)"""
    if lay.instances == 1:
        return r // lay.per_item, (r % lay.per_item) * record_bytes, record_bytes, 0
    first = instance * lay.item_bytes
    return r, 0, min(record_bytes - first, lay.item_bytes), first


def trials_of(lay: Layout, offset: int, nbytes: int) -> range:
    """the trials whose polynomial holds a byte of [offset, offset + nbytes) of an item's stream"""
    pb = 256 * lay.coeff_bits
    return range(offset // pb, -(-(offset + nbytes) // pb))


def splice(coeffs: np.ndarray, w: int, offset: int, data) -> np.ndarray:
    """item [trials][2048] with bytes [offset, offset + len(data)) of its stream replaced: bit b of the stream is bit b % w of coefficient b // w of
    the flat [trials * 2048] coefficients; every other bit of every coefficient stays"""
    coeffs = np.asarray(coeffs)
    bits = bits_of(coeffs, w)
    new = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little")
    assert 8 * offset + len(new) <= len(bits)
    bits[8 * offset:8 * offset + len(new)] = new
    return coeffs_of(bits, w).reshape(coeffs.shape)


def cut(coeffs: np.ndarray, w: int, offset: int, nbytes: int) -> np.ndarray:
    """bytes [offset, offset + nbytes) of an item's stream"""
    c0, c1 = 8 * offset // w, -(-8 * (offset + nbytes) // w)  # the coefficients the range touches
    start = 8 * offset - c0 * w
    return np.packbits(bits_of(np.asarray(coeffs).reshape(-1)[c0:c1], w)[start:start + 8 * nbytes], bitorder="little")


def item_stream(lay: Layout, record_bytes: int, records: np.ndarray, instance: int = 0) -> np.ndarray:
    """records [n][S] (n a multiple of per_item, starting at a multiple of it) -> the items instance `instance` holds, [items][item_bytes], padding zero;
    trial t's polynomial of item i is bytes [t * 256 w, (t + 1) * 256 w) of row i"""
    records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, record_bytes)
    n_items = len(records) // lay.per_item
    out = np.zeros((n_items, lay.item_bytes), dtype=np.uint8)
    for k in range(n_items * lay.per_item):
        item, off, nb, first = place(lay, record_bytes, k, instance)
        out[item, off:off + nb] = records[k, first:first + nb]
    return out


def stream_coeffs(stream: np.ndarray, w: int, trials: int) -> np.ndarray:
    """an item stream (whole items) -> coefficients [items][trials][2048]"""
    return coeffs_of(np.unpackbits(np.ascontiguousarray(stream, dtype=np.uint8).reshape(-1), bitorder="little"), w).reshape(-1, trials, N)
