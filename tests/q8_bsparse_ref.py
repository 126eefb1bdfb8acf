"""A numpy restatement of the block-sparse fp8 contract (include/mcamd.h), test-side only: mcamd_pack_q8's byte
matrix from OIHW codes, and the chunk lists of such a matrix."""
import numpy as np

FILTERS = 64      # filters per tile = the N tile of the block-sparse fp8 forward
CHUNK = 64        # bytes per K chunk = one (channel block of 64, tap) pair


def pack_bytes(w8):
    """uint8 [round_up(cout, 256)][khw * cin] packing of OIHW e4m3 codes with cin % 64 == 0: column
    kpos(t, c) = (c / 64) * khw * 64 + t * 64 + c % 64; pad rows 0x00."""
    w8 = np.asarray(w8, np.uint8)
    cout, cin = w8.shape[:2]
    assert cin % CHUNK == 0
    v = w8.reshape(cout, cin // CHUNK, CHUNK, -1)
    khw = v.shape[3]
    out = np.zeros(((cout + 255) // 256 * 256, khw * cin), np.uint8)
    out[:cout] = v.transpose(0, 1, 3, 2).reshape(cout, khw * cin)
    return out


def chunk_lists(packed, cout):
    """(count int32[ntiles], list int32[ntiles][nchunks]) of a packed byte matrix: per tile of 64 rows the chunks q with any
    byte b, b & 0x7f != 0 (0x00 and 0x80 are the two e4m3 zeros), in columns [64 q, 64 q + 64), ascending; entries behind the
    count are 0."""
    packed = np.asarray(packed, np.uint8)
    ntiles, nchunks = (cout + FILTERS - 1) // FILTERS, packed.shape[1] // CHUNK
    count = np.zeros(ntiles, np.int32)
    lst = np.zeros((ntiles, nchunks), np.int32)
    for nt in range(ntiles):
        rows = packed[FILTERS * nt:FILTERS * nt + FILTERS].reshape(-1, nchunks, CHUNK)
        q = np.nonzero(((rows & 0x7F) != 0).any(axis=(0, 2)))[0]
        count[nt] = q.shape[0]
        lst[nt, :q.shape[0]] = q
    return count, lst


def kept_fraction(packed, cout):
    """sum(count) / (tiles x chunks): what Engine.fp8_block_kept reports for the layer."""
    count, lst = chunk_lists(packed, cout)
    return float(count.sum()) / float(lst.size)
