"""PackSet: the opt-in (DD_PACK_MANY=1) batching of a network's dd_conv3x3_mfma weight packs into one launch per forward pass, for
functions.MfmaConvFn (functions.py imports this module, never the other way round).

OPEN: the hooks are registered whether or not DD_PACK_MANY is set; with it a member's pack_b is ONE buffer, so a later
forward pass rewrites what an earlier pass saved for its backward (a race under a multi-stream backward, stale if the weights moved in
between); _ACTIVE_PACK_SETS is process-global, not thread-local.
"""
import os

import torch

from . import lib as L


class _PackEntry:
    __slots__ = ("weight", "pack_f", "pack_b", "fresh", "sig")

    def __init__(self, weight, pack_f, pack_b):
        self.weight, self.pack_f, self.pack_b, self.fresh = weight, pack_f, pack_b, 0
        self.sig = (weight.data_ptr(), tuple(weight.stride()), tuple(weight.shape))


class PackSet:
    """The dd_conv3x3_mfma weight packs of ONE network module, made by one launch at the top of its forward pass (round 6: the step had 62
    pack launches of 4-8 us, each in front of its convolution on the network's stream; dd_conv3x3_mfma_pack_many makes a network's in one).
    A layer joins the set the first time MfmaConvFn.forward runs inside the module's forward (it packs alone that time, its buffers become
    the set's); from the next pass on the module's forward-pre hook packs every member and marks it fresh, the layer takes the fresh pack
    ONCE -- any other call (outside the module's forward, a second use in one pass, a weight that moved) packs alone as before, so a pack
    is never older than the forward pass that uses it.  Job tables and pack buffers are never freed: captured graphs hold their addresses."""

    def __init__(self):
        self.entries = {}          # id(weight) -> _PackEntry
        self.tables = {}           # (with data-gradient packs?, members' signatures) -> (jobs, block_job, n_blocks)
        self.retired = []          # buffers replaced by an upgrade (a member that later needed its data-gradient pack)

    def pack_all(self):
        if not self.entries:
            return
        with_b = torch.is_grad_enabled()
        members = list(self.entries.values())
        # a member whose weight moved (another device, another layout) leaves the set: its layer re-joins with the next call
        for e in members:
            if e.sig != (e.weight.data_ptr(), tuple(e.weight.stride()), tuple(e.weight.shape)):
                self.retired.append(self.entries.pop(id(e.weight)))
        members = list(self.entries.values())
        if not members:
            return
        sig = tuple((e.sig, e.pack_f.data_ptr(), 0 if e.pack_b is None else e.pack_b.data_ptr()) for e in members)
        table = self.tables.get((with_b, sig))
        lib = L.load()
        if table is None:
            if torch.cuda.is_current_stream_capturing():
                return             # no host-to-device copy inside a capture: this pass packs layer by layer
            for mode in (True, False):          # both tables at once: a tape-free pass of the same members may first come inside a capture
                self.tables[(mode, sig)] = self._table(lib, members, mode)
            table = self.tables[(with_b, sig)]
        L.check(lib.dd_conv3x3_mfma_pack_many(table[0].data_ptr(), table[1].data_ptr(), table[2], L.current_stream()), "dd_conv3x3_mfma_pack_many")
        _PACK_MANY_LAUNCHES[0] += 1
        for e in members:
            e.fresh = 2 if (with_b and e.pack_b is not None) else 1

    @staticmethod
    def _table(lib, members, with_b):
        words = lib.dd_conv3x3_mfma_pack_many_job_words()
        jobs, owner, first = [], [], 0
        for n, e in enumerate(members):
            cout, cin = e.weight.shape[:2]
            has_b = with_b and e.pack_b is not None
            sw = e.weight.stride()
            row = [e.weight.data_ptr(), sw[0], sw[1], sw[2], sw[3], cout, cin, e.pack_f.data_ptr(), e.pack_b.data_ptr() if has_b else 0, first]
            assert len(row) == words
            jobs.append(row)
            nb = lib.dd_conv3x3_mfma_pack_many_blocks(cout, cin, 1, 1 if has_b else 0)
            owner += [n] * nb
            first += nb
        dev = members[0].weight.device
        return torch.tensor(jobs, dtype=torch.int64).to(dev), torch.tensor(owner, dtype=torch.int32).to(dev), first

    def take(self, weight, need_b):
        """The fresh pack of this weight, once: (pack_fwd, pack_bwd_data) or None."""
        e = self.entries.get(id(weight))
        if e is None or e.weight is not weight or e.fresh < (2 if need_b else 1):
            return None
        if e.sig != (weight.data_ptr(), tuple(weight.stride()), tuple(weight.shape)):
            return None
        e.fresh = 0
        return e.pack_f, (e.pack_b if need_b else None)

    def join(self, weight, pack_f, pack_b):
        old = self.entries.get(id(weight))
        if old is not None:
            if old.weight is weight and old.sig == (weight.data_ptr(), tuple(weight.stride()), tuple(weight.shape)) and (pack_b is None or old.pack_b is not None):
                return             # a second use in one pass, or a tape-free pass of a member: nothing to learn
            self.retired.append(old)
        self.entries[id(weight)] = _PackEntry(weight, pack_f, pack_b)

    def end(self):
        for e in self.entries.values():
            e.fresh = 0


_PACK_SETS = {}                # id(module) -> (weak reference to the module, PackSet)
_ACTIVE_PACK_SETS = []         # the sets of the modules whose forward is running (innermost last)
_PACK_MANY_LAUNCHES = [0]


def pack_many_launches():
    """How many times a network's packs were made by one dd_conv3x3_mfma_pack_many launch in this process."""
    return _PACK_MANY_LAUNCHES[0]


def _pack_many_on():
    # OPT-IN: measured neutral in the headline step (341.7 / 341.3 img/s with it, 342.2 / 343.5 without, same box back to back) although it
    # takes 54 launches and 0.32 ms of kernel time out of the step -- the packs were never on the step's critical path, and one 60 us
    # launch at the head of an encoder delays its first convolution more than the 4-8 us packs interleaved with other streams' work did
    return os.environ.get("DD_PACK_MANY", "0") == "1"


def pack_weights_once_per_forward(module):
    """Make `module` (a network: an encoder, a decoder) pack the weights of its dd_conv3x3_mfma layers in ONE launch at the top of every
    forward pass (PackSet) when DD_PACK_MANY=1.  Returns the module.  Default (0): every layer packs in front of its own convolution."""
    import weakref
    if id(module) in _PACK_SETS and _PACK_SETS[id(module)][0]() is module:
        return module
    ps = PackSet()
    _PACK_SETS[id(module)] = (weakref.ref(module, lambda _r, k=id(module): _PACK_SETS.pop(k, None)), ps)

    def before(_m, _inputs):
        _ACTIVE_PACK_SETS.append(ps)
        if _pack_many_on():
            ps.pack_all()

    def after(_m, _inputs, _outputs):
        ps.end()
        if _ACTIVE_PACK_SETS and _ACTIVE_PACK_SETS[-1] is ps:
            _ACTIVE_PACK_SETS.pop()

    module.register_forward_pre_hook(before)
    module.register_forward_hook(after, always_call=True)
    return module
