"""Guard words around device buffers, and the memory contract of include/ossid_hip.h checked through them.

The header's first convention: the caller owns all memory, workspaces included, with sizes from the size queries. The
wrappers never hand a kernel a buffer of exactly the queried size (allocation floors, grow-only scratch, the caching
allocator's rounding), and a fresh process usually sees zeroed device memory. `Guarded` is a buffer of exactly the size
asked for between two runs of guard bytes; `run_contract` runs one entry three times -- a generous zeroed workspace, then
exactly the queried bytes filled with 0xFF and with 0x7F -- and wants byte-identical outputs, untouched guards, a refusal
one byte short, and run A's outputs within the entry's own existing bound of its reference.

Plain helper module: tests/workspace_cases.py builds the `Contract`s, the test_workspace_contract*_gpu.py files run them."""
import torch

GUARD_BYTE = 0xC3
OUT_FILL = 0xA5
LEAD = 4096
EINVAL, ELAUNCH = -22, -5

# a HIP error anywhere ends the file: nothing is launched on a device that has faulted
_STOPPED = []


class Guarded:
    """One uint8 CUDA allocation [lead guard | payload | trail guard]: the payload (`nbytes` bytes of `fill`) starts at an
    `align`-byte boundary, the guards hold GUARD_BYTE; the lead guard is 4 KiB (plus the bytes the alignment takes), the
    trail guard at least max(64 KiB, nbytes): an overrun of up to twice the payload lands in memory the test owns."""

    def __init__(self, nbytes, fill, align=256):
        nbytes = int(nbytes)
        trail = max(64 << 10, nbytes)
        self.whole = torch.full((LEAD + align + nbytes + trail,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.off = LEAD + (-(self.whole.data_ptr() + LEAD)) % align
        self.nbytes = nbytes
        self.payload = self.whole[self.off:self.off + nbytes]
        self.payload.fill_(fill)
        self.ptr = self.whole.data_ptr() + self.off
        assert self.ptr % align == 0

    def view(self, dtype):
        return self.payload.view(dtype)

    def put(self, t):
        """Copies a contiguous CUDA tensor of exactly nbytes into the payload."""
        src = t.contiguous().view(-1).view(torch.uint8)
        assert src.numel() == self.nbytes, (src.numel(), self.nbytes)
        self.payload.copy_(src)

    def intact(self):
        """Both guards still hold GUARD_BYTE (compared on the device)."""
        lead, trail = self.whole[:self.off], self.whole[self.off + self.nbytes:]
        return bool(((lead == GUARD_BYTE).all() & (trail == GUARD_BYTE).all()).item())


class Span:
    """A (ptr, nbytes) pair as an entry sees it: what `run` receives for a workspace, possibly lying about either."""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class Contract:
    """One consuming entry (or entries run as a unit) at one shape.

    workspaces  name -> queried bytes (usually one, "ws")
    outputs     name -> bytes; `init` name -> CUDA tensor copied in instead of the 0xA5 prefill (an accumulator)
    run(ws, out) -> status; ws / out map names to objects with .ptr and .nbytes
    anchor(out)  checks run A's outputs against the entry's own reference (out: name -> Guarded); None = a comment at the
                 case names the existing test that pins this very shape
    short       names of the workspaces whose byte count the entry takes: one byte less must be refused
    misalign    names of the workspaces whose alignment the header states: a pointer off by 4 must be refused
    expect      the status all three runs must return (OSSID_EINVAL for an entry a build switch turns off)"""

    def __init__(self, name, workspaces, outputs, run, anchor=None, init=None, short=(), misalign=(), align=256, expect=0):
        self.name, self.workspaces, self.outputs, self.run, self.anchor = name, dict(workspaces), dict(outputs), run, anchor
        self.init, self.short, self.misalign, self.align, self.expect = dict(init or {}), tuple(short), tuple(misalign), align, expect


def ready():
    """Called before anything touches the device: after a HIP error the file stops there."""
    assert not _STOPPED, "an earlier case reported a HIP error: nothing more is launched from this file"


def sync():
    try:
        torch.cuda.synchronize()
    except Exception:
        _STOPPED.append(True)
        raise


def _outputs(c):
    outs = {k: Guarded(n, OUT_FILL) for k, n in c.outputs.items()}
    for k, t in c.init.items():
        outs[k].put(t)
    return outs


def _call(c, ws, outs):
    rc = c.run(ws, outs)
    if rc == ELAUNCH:
        _STOPPED.append(True)
    sync()
    return rc


def run_contract(c):
    """Section 4 of the contract for one Contract (see the module docstring). Returns {workspace name: queried bytes}."""
    ready()
    for k, n in c.workspaces.items():
        assert n > 0, "%s: the query for %s returned %d" % (c.name, k, n)
    first = None
    for tag, fill, size in (("A", 0x00, lambda n: 2 * n + (1 << 20)), ("B", 0xFF, lambda n: n), ("C", 0x7F, lambda n: n)):
        ws = {k: Guarded(size(n), fill, c.align) for k, n in c.workspaces.items()}
        outs = _outputs(c)
        rc = _call(c, ws, outs)
        assert rc == c.expect, "%s run %s: status %d, expected %d" % (c.name, tag, rc, c.expect)
        for k, g in list(ws.items()) + list(outs.items()):
            assert g.intact(), "%s run %s: the guard words around `%s` (%d bytes) were overwritten" % (c.name, tag, k, g.nbytes)
        if first is None:
            first = outs
            if c.expect == 0 and c.anchor is not None:
                c.anchor(outs)
        else:
            for k in outs:
                diff = int((outs[k].payload != first[k].payload).sum())
                assert diff == 0, ("%s: output `%s` of run %s (workspace of exactly the queried size, filled with 0x%02X) differs "
                                   "from run A in %d of %d bytes" % (c.name, k, tag, fill, diff, outs[k].nbytes))
    if c.expect != 0:
        for k, g in first.items():
            if k not in c.init:
                assert bool((g.payload == OUT_FILL).all()), "%s: refused, yet `%s` was written" % (c.name, k)
        return dict(c.workspaces)
    for what, names in (("short", c.short), ("misaligned", c.misalign)):
        for name in names:
            ws = {k: Guarded(n + 8, 0x00, c.align) for k, n in c.workspaces.items()}
            seen = {k: Span(g.ptr, c.workspaces[k]) for k, g in ws.items()}
            seen[name] = Span(ws[name].ptr, c.workspaces[name] - 1) if what == "short" else Span(ws[name].ptr + 4, c.workspaces[name])
            outs = _outputs(c)
            rc = _call(c, seen, outs)
            assert rc == EINVAL, "%s: a %s workspace `%s` returned %d, not OSSID_EINVAL" % (c.name, what, name, rc)
            for k, g in outs.items():
                assert g.intact()
                if k not in c.init:
                    assert bool((g.payload == OUT_FILL).all()), "%s: refused, yet `%s` was written" % (c.name, k)
    return dict(c.workspaces)
