"""Python restatement of the per-tensor tables of csrc/param_tables.hip, from layout.param_specs alone: the tensors, the AdamItem of
each (csrc/ops.h), the slice counts, and the (first, end) pairs every range entry point must refuse."""
import ctypes

SLICE = 8192            # csrc/ops.h M2F_PARAM_SLICE
TABLE_BYTES = 64 * 1024  # the region behind the parameter shadows: AdamItem[n] | int tile_begin[n + 1]


class AdamItemC(ctypes.Structure):
    """csrc/ops.h AdamItem."""
    _fields_ = [("off", ctypes.c_longlong), ("soff", ctypes.c_longlong), ("soff_t", ctypes.c_longlong),
                ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("tile_begin", ctypes.c_int), ("tiles_c", ctypes.c_int)]


def tensors(cfg):
    """-> ([(offset, numel, shape)] of the unique parameter tensors in flat order, total elements)."""
    from mer_amd import layout
    specs, total = layout.param_specs(cfg)
    return [(s.offset, s.numel, s.shape) for s in specs if not s.alias_of], total


def n_slices(cfg):
    return sum((n + SLICE - 1) // SLICE for _, n, _ in tensors(cfg)[0])


def items(cfg):
    """-> ([(off, rows, cols, tiles_c, tile_begin)] per tensor, prefix [n + 1]): a matrix in 64 x 64 tiles, a 1-D tensor with its pad up
    to the next tensor as `cols` elements in tiles of 4096."""
    ts, total = tensors(cfg)
    out, prefix, tiles = [], [], 0
    for i, (off, numel, shape) in enumerate(ts):
        prefix.append(tiles)
        if len(shape) == 2:
            rows, cols = shape
            tiles_c = (cols + 63) // 64
            out.append((off, rows, cols, tiles_c, tiles))
            tiles += (rows + 63) // 64 * tiles_c
        else:
            cols = (ts[i + 1][0] if i + 1 < len(ts) else total) - off
            out.append((off, 0, cols, 1, tiles))
            tiles += (cols + 4095) // 4096
    prefix.append(tiles)
    return out, prefix


def bad_ranges(cfg):
    """{why: (first, end)}: none of them is a run of whole parameter tensors."""
    ts, total = tensors(cfg)
    offs = [o for o, _, _ in ts]
    padded = next(i for i, (o, n, _) in enumerate(ts[:-1]) if n % 64)        # a tensor with a pad behind it, not the last one
    bad = {
        "first inside a tensor": (offs[0] + 4, -1),
        "first in a pad": (offs[padded] + ts[padded][1] + 4, -1),
        "end == first": (offs[2], offs[2]),
        "end < first": (offs[3], offs[1]),
        "end inside a tensor": (offs[0], offs[1] + 4),
        "first past the last tensor": (total, -1),
    }
    assert offs[padded] + ts[padded][1] + 4 < offs[padded + 1] and ts[0][1] > 4 and ts[1][1] > 4
    return bad


RANGE_WORDING = ("[first, end) must start at a parameter tensor and hold at least one",
                 "`end` must be the offset of a parameter tensor (or < 0)")
