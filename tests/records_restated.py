"""The record layout of include/spiral_gpu.h ("Records") and the bit-level splice, restated in numpy for the record tests.  Nothing here calls the
library under test: the layout is arithmetic on (p_db, nu1, nu2, S), the splice works on plaintext coefficients, one bit at a time.

A plaintext is [2][2][2048] coefficients (polynomial (m, c)); its stream is the little-endian string of w-bit coefficients, polynomial (m, c) first
coefficient at bit (m * 2 + c) * 2048 * w, which is what read_db_items(w) returns for a power-of-two p_db."""
from dataclasses import dataclass

import numpy as np

N = 2048


@dataclass(frozen=True)
class Layout:
    coeff_bits: int  # w
    item_bytes: int
    per_item: int
    instances: int
    capacity: int


def layout(p_db: int, nu1: int, nu2: int, record_bytes: int) -> Layout:
    """None where the layout is refused (more than 16 instances)"""
    w = p_db.bit_length() - 1  # floor(log2 p_db)
    item_bytes = 1024 * w
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


def bits_of(coeffs, w: int) -> np.ndarray:
    """plaintext coefficients (any shape) -> the bits of their stream, one uint8 per bit"""
    v = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1)
    return ((v[:, None] >> np.arange(w, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)


def coeffs_of(bits: np.ndarray, w: int) -> np.ndarray:
    """the inverse of bits_of, flat"""
    return (bits.reshape(-1, w).astype(np.uint64) << np.arange(w, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def stream_of(coeffs, w: int) -> np.ndarray:
    """plaintext coefficients -> their stream as bytes"""
    return np.packbits(bits_of(coeffs, w), bitorder="little")


def stream_coeffs(stream: np.ndarray, w: int) -> np.ndarray:
    """an item stream (whole plaintexts) -> coefficients [items][2][2][2048]"""
    return coeffs_of(np.unpackbits(np.ascontiguousarray(stream, dtype=np.uint8).reshape(-1), bitorder="little"), w).reshape(-1, 2, 2, N)


def splice(coeffs: np.ndarray, w: int, offset: int, data) -> np.ndarray:
    """plaintext [2][2][2048] with bytes [offset, offset + len(data)) of its stream replaced: bit b of the range lands in coefficient b // w, bit b % w;
    every other bit of every coefficient stays"""
    bits = bits_of(coeffs, w)
    new = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little")
    assert 8 * offset + len(new) <= len(bits)
    bits[8 * offset:8 * offset + len(new)] = new
    return coeffs_of(bits, w).reshape(2, 2, N)


def cut(coeffs: np.ndarray, w: int, offset: int, nbytes: int) -> np.ndarray:
    """bytes [offset, offset + nbytes) of a plaintext's stream"""
    c0, c1 = 8 * offset // w, -(-8 * (offset + nbytes) // w)  # the coefficients the range touches
    start = 8 * offset - c0 * w
    return np.packbits(bits_of(np.asarray(coeffs).reshape(-1)[c0:c1], w)[start:start + 8 * nbytes], bitorder="little")


def item_stream(lay: Layout, record_bytes: int, records: np.ndarray, instance: int = 0) -> np.ndarray:
    """records [n][S] (n a multiple of per_item, starting at a multiple of it) -> the items instance `instance` holds, [items][item_bytes], padding zero"""
    records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, record_bytes)
    n_items = len(records) // lay.per_item
    out = np.zeros((n_items, lay.item_bytes), dtype=np.uint8)
    if lay.instances == 1:  # item i: its per_item records back to back from byte 0 (place() for every record at once)
        out[:, :lay.per_item * record_bytes] = records[:n_items * lay.per_item].reshape(n_items, lay.per_item * record_bytes)
        return out
    for k in range(len(records)):
        item, off, nb, first = place(lay, record_bytes, k, instance)
        out[item, off:off + nb] = records[k, first:first + nb]
    return out
