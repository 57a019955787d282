"""Guard-banded device buffers for the GPU tests: catch reads and writes beyond a tensor's ends, and reads of memory nobody wrote.

`guarded(shape, dtype, role)` returns a contiguous view inside a larger buffer with at least GUARD_BYTES (1 MiB) of guard band on
each side -- anything short of a wild pointer lands inside it instead of in the allocator's slack.

  role "in"   guards = all-ones bytes (NaN in fp16, fp32 and e4m3): a kernel that reads past an input multiplies NaN into its result.
              The payload is all-ones too until the caller copies its data in (`gin` does both).
  role "out"  guards and payload = a sentinel: all-ones bytes for float outputs, so "every element was written" stays a finiteness
              check; the odd byte 0xA5 for integer outputs.
  role "ws"   a workspace: guards all-ones, payload filled with `payload_fill` (one byte value; the poisoned-workspace tests use
              0x00, 0xFF and 0x7B).

`skew` puts the payload at (a multiple of 256 B) + skew bytes: skew=16 is exactly the alignment include/lunaris_hip.h promises to
the kernels, instead of the 512 B torch's allocator gives every tensor.

`check_guards(*views)` compares every guard band, on the device and bit for bit, with its fill and names the first byte that
differs.  Pass the tensors `guarded` returned (or views of them: the bands are found through the shared storage).
"""
import torch

GUARD_BYTES = 1 << 20
ONES = 0xFF
INT_SENTINEL = 0xA5
ALIGN = 16                 # the ABI's promise (include/lunaris_hip.h): every tensor pointer is 16-byte aligned

_bands = {}                # storage address -> (payload byte offset, payload bytes, guard fill byte, total bytes)


def guarded(shape, dtype, role, skew=0, payload_fill=None, device="cuda"):
    if isinstance(shape, int):
        shape = (shape,)
    assert role in ("in", "out", "ws"), role
    item = torch.empty(0, dtype=dtype).element_size()
    n = 1
    for d in shape:
        n *= int(d)
    nbytes = n * item
    assert skew >= 0 and skew % item == 0 and skew % ALIGN == 0, f"skew {skew}: a multiple of {ALIGN} B and of the element size"
    total = GUARD_BYTES + 256 + skew + nbytes + GUARD_BYTES
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    base = buf.data_ptr()
    off = (base + GUARD_BYTES + 255) // 256 * 256 - base + skew
    assert off >= GUARD_BYTES and total - (off + nbytes) >= GUARD_BYTES
    if role == "out" and not dtype.is_floating_point:
        guard_fill = INT_SENTINEL
    else:
        guard_fill = ONES
    buf.fill_(guard_fill)
    if role == "ws":
        buf[off:off + nbytes].fill_(ONES if payload_fill is None else payload_fill)
    elif payload_fill is not None:
        buf[off:off + nbytes].fill_(payload_fill)
    _bands[buf.untyped_storage().data_ptr()] = (off, nbytes, guard_fill, total)
    view = buf[off:off + nbytes].view(dtype).view(*shape)
    assert view.is_contiguous() and (view.data_ptr() - skew) % 256 == 0
    return view


def gin(t, skew=0, dtype=None):
    """A guarded "in" tensor holding a copy of `t` (any device), optionally converted to `dtype`."""
    t = t.contiguous()
    g = guarded(tuple(t.shape), dtype or t.dtype, "in", skew)
    g.copy_(t)
    return g


def _first_diff(band, fill):
    bad = band != fill
    if not bool(bad.any()):
        return None
    idx = torch.nonzero(bad)
    return int(idx[0]), int(idx[-1]), int(idx.numel())


def check_guards(*views):
    """Every guard band of every view still holds its fill, bit for bit; None entries are skipped."""
    for k, v in enumerate(views):
        if v is None:
            continue
        st = v.untyped_storage()
        key = st.data_ptr()
        assert key in _bands, f"check_guards: argument {k} did not come from guarded()"
        off, nbytes, fill, total = _bands[key]
        assert st.nbytes() == total, f"check_guards: argument {k} did not come from guarded() (stale band record)"
        whole = torch.empty(0, dtype=torch.uint8, device=v.device).set_(st)
        what = f"argument {k} ({tuple(v.shape)} {v.dtype}, payload {nbytes} B)"
        hi = _first_diff(whole[off + nbytes:], fill)
        assert hi is None, (f"guard band ABOVE {what} changed: first differing byte {hi[0]} B past the payload's end "
                            f"(last {hi[1]} B past, {hi[2]} bytes differ): a write beyond the tensor")
        lo = _first_diff(whole[:off], fill)
        assert lo is None, (f"guard band BELOW {what} changed: nearest differing byte {off - lo[1]} B before the payload's start "
                            f"(farthest {off - lo[0]} B before, {lo[2]} bytes differ): a write in front of the tensor")


def written(*views):
    """No element of a float "out" view still holds the all-ones sentinel (NaN), i.e. every element was written with a finite value."""
    for k, v in enumerate(views):
        if v is not None:
            assert bool(torch.isfinite(v.float()).all()), f"output {k} {tuple(v.shape)}: elements left unwritten (sentinel) or not finite"
