"""The two host-side policies of the training engine that have one owner each (disconet_amd/train.py): how long a measured
power-of-two lift is used (_Lifts) and which packed weight forms the one-launch packs hold and serve (_PackedForms).  No GPU, no
library: ops.PackSet is replaced by a fake that records what it is given."""
import ctypes

import pytest
import torch

from disconet_amd import ops, train
from disconet_amd.train import _Lifts, _PackedForms


# ---- lifts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measured_at", [0, 100, 1000])
def test_a_lift_is_fresh_for_63_steps_either_way_and_stale_at_64(measured_at):
    ent = (4.0, measured_at)
    assert train._LIFT_REFRESH_STEPS == 64
    for delta in (0, 1, 63):
        assert _Lifts.fresh(ent, measured_at + delta) and _Lifts.fresh(ent, measured_at - delta), delta      # backwards: a resumed run
    for delta in (64, 65, 10000):
        assert not _Lifts.fresh(ent, measured_at + delta) and not _Lifts.fresh(ent, measured_at - delta), delta
    assert not _Lifts.fresh(None, measured_at)


def test_dropping_one_kind_of_lift_leaves_the_other():
    lifts = _Lifts()
    lifts.set_weight(("p", 0), 8.0, 3)
    lifts.set_dz("conv1_1", 0.01, 3)
    dz_table = lifts.dz
    lifts.drop_dz()
    assert lifts.dz == {} and lifts.dz is dz_table and lifts.weights == {("p", 0): (8.0, 3)}      # (the engine's _dz_lift IS that dict)
    lifts.set_dz("conv1_1", 0.01, 4)
    lifts.drop_weights()
    assert lifts.weights == {} and list(lifts.dz) == ["conv1_1"] and lifts.dz["conv1_1"][1] == 4


def test_only_a_parentless_temporary_starts_the_weight_table_over_and_only_past_256_entries():
    lifts = _Lifts()
    for i in range(300):                                  # parameter entries alone never evict anything
        lifts.set_weight(("p", i), 2.0, 0)
    assert len(lifts.weights) == 300
    lifts = _Lifts()
    for i in range(200):
        lifts.set_weight(("p", i), 2.0, 0)
    for i in range(56):
        lifts.set_weight(("t", i), 2.0, 0, temporary=True)
    assert len(lifts.weights) == 256
    lifts.set_weight(("t", 56), 2.0, 0, temporary=True)  # 256 entries: not more than 256, nothing is dropped
    assert len(lifts.weights) == 257
    assert lifts.set_weight(("t", 57), 4.0, 9, temporary=True) == (4.0, 9)      # more than 256: the table starts over
    assert lifts.weights == {("t", 57): (4.0, 9)}


def test_a_dz_measurement_sets_the_lift_that_puts_it_near_2_to_the_8_and_a_useless_one_removes_the_entry():
    lifts = _Lifts()
    lifts.set_dz("a", 1.0, 5)
    lifts.set_dz("b", 3e-5, 5)           # 2^-16 <= 3e-5 < 2^-15
    lifts.set_dz("c", 700.0, 5)          # 2^9 <= 700 < 2^10
    assert lifts.dz == {"a": (256.0, 5), "b": (2.0 ** 24, 5), "c": (0.5, 5)}
    for name, bad in (("a", 0.0), ("b", float("nan")), ("c", float("inf"))):
        lifts.set_dz(name, bad, 6)
        assert name not in lifts.dz
    lifts.set_dz("never_there", float("nan"), 6)
    assert lifts.dz == {}
    lifts.set_dz("tiny", 1e-300, 7)      # the exponent is clamped
    assert lifts.dz["tiny"] == (2.0 ** 100, 7)


# ---- packed weight forms ---------------------------------------------------------------------------------------------------
class _Desc(ctypes.Structure):
    _fields_ = [("c0", ctypes.c_int), ("c_out", ctypes.c_int), ("ksize", ctypes.c_int)]


class _FakePackSet:
    """what _PackedForms uses of ops.PackSet: supported(), buffers, run(), n"""
    built = []                 # every set, in the order it was built
    unsupported_c_out = 7

    def __init__(self, jobs, device, engine="sp"):
        self.jobs, self.device, self.engine, self.n = list(jobs), device, engine, len(jobs)
        self.buffers = [("image", engine, len(_FakePackSet.built), i) for i in range(self.n)]
        self.runs = []
        self.fail = False
        _FakePackSet.built.append(self)

    @classmethod
    def supported(cls, d, engine="sp"):
        return d.c_out != cls.unsupported_c_out

    def run(self, wmuls):
        if self.fail:
            raise RuntimeError("pack launch failed")
        self.runs.append(list(wmuls))


@pytest.fixture
def fake_packset(monkeypatch):
    _FakePackSet.built = []
    monkeypatch.setattr(ops, "PackSet", _FakePackSet)
    return _FakePackSet


class _Asker:
    """asks a _PackedForms for forms the way the engine's _packed_form does, counting the single packs"""

    def __init__(self, enabled=True):
        self.forms = _PackedForms("dev", enabled=enabled)
        self.singles = 0
        self.w = torch.zeros(8, 4, 3, 3)
        self.lifted = torch.zeros(1)

    def single(self):
        self.singles += 1
        return "single"

    def get(self, off=0, mode=0, c_out=8, ci_first=0, n_in=0, lift=False, engine="sp", c0=4):
        return self.forms.get(off, self.w, mode, _Desc(c0, c_out, 3), ci_first, n_in, self.lifted if lift else None, engine, self.single)

    def forward(self, generation):
        self.forms.begin_forward(generation, lambda p: 16.0)


def test_a_form_is_packed_singly_in_the_forward_that_first_asks_and_served_from_the_set_from_the_next(fake_packset):
    a = _Asker()
    a.forward(1)
    assert a.forms.sizes() == {} and fake_packset.built == []
    assert a.get(lift=True) == "single" and a.get(lift=True) == "single" and a.singles == 2      # (asked twice in forward 1: queued once)
    assert a.get(off=640, engine="nhwc") == "single"
    assert a.forms.sizes() == {}
    a.forward(2)
    assert a.forms.sizes() == {"sp": 1, "nhwc": 1}
    sp, nhwc = fake_packset.built
    assert (sp.engine, sp.device, sp.runs) == ("sp", "dev", [[16.0]]) and nhwc.runs == [[1.0]]      # no lift Parameter: 1
    d, w3, mode, cin_total, ci_first, n_in = sp.jobs[0]
    assert (d.c0, d.c_out, d.ksize, tuple(w3.shape), mode, cin_total, ci_first, n_in) == (4, 8, 3, (8, 4, 9), 0, 4, 0, 0)
    assert w3.data_ptr() == a.w.data_ptr()                # the weights are read in place
    assert a.get(lift=True) is sp.buffers[0] and a.get(off=640, engine="nhwc") is nhwc.buffers[0] and a.singles == 3
    a.forward(3)                                          # nothing new: the same sets run again
    assert fake_packset.built == [sp, nhwc] and sp.runs == [[16.0], [16.0]]
    assert a.get(lift=True) is sp.buffers[0] and a.singles == 3


def test_an_image_is_served_only_in_the_forward_that_packed_it(fake_packset):
    a = _Asker()
    a.forward(1)
    a.get()
    a.forward(2)
    (s,) = fake_packset.built
    assert a.get() is s.buffers[0]
    s.fail = True
    with pytest.raises(RuntimeError):
        a.forward(3)                                      # the set did not run in forward 3: its images hold forward 2's weights
    assert a.get() == "single" and a.singles == 2
    s.fail = False
    a.forward(4)
    assert a.get() is s.buffers[0] and fake_packset.built == [s]


def test_a_form_nobody_asked_for_in_eight_forwards_leaves_the_next_set_and_one_asked_for_at_the_eighth_stays(fake_packset):
    a = _Asker()
    a.forward(1)
    a.get(off=0)
    a.get(off=100)
    a.forward(2)
    assert a.forms.sizes() == {"sp": 2}
    for g in range(3, 10):                                # forwards 2 .. 9: nobody asks for either
        a.forward(g)
    assert len(fake_packset.built) == 1
    a.get(off=100)                                        # forward 9: the eighth after forward 1
    a.get(off=200)                                        # a new form: the next forward rebuilds the set
    a.forward(10)
    assert a.forms.sizes() == {"sp": 2}
    assert sorted(k[0] for k in a.forms._engines["sp"].jobs) == [100, 200] and fake_packset.built[-1].n == 2      # off 0: asked for 9 forwards ago
    n = a.singles
    assert a.get(off=0) == "single" and a.singles == n + 1      # ... and queued again like a new form
    a.forward(11)
    assert a.forms.sizes() == {"sp": 3}
    # exactly eight forwards unused is still kept
    b = _Asker()
    b.forward(1)
    b.get(off=0)
    b.forward(2)
    for g in range(3, 9):
        b.forward(g)
    b.get(off=300)                                        # forward 8
    b.forward(9)                                          # off 0 was asked for in forward 1: 9 - 1 = 8, kept
    assert b.forms.sizes() == {"sp": 2}


def test_an_unsupported_form_is_never_queued_and_packed_singly_every_time(fake_packset):
    a = _Asker()
    for g in range(1, 5):
        a.forward(g)
        assert a.get(c_out=fake_packset.unsupported_c_out) == "single"
    assert a.singles == 4 and a.forms.sizes() == {} and fake_packset.built == []
    fs = a.forms._engines["sp"]
    assert not fs.jobs and not fs.pending and len(fs.single) == 1
    # a weight that is not in the flat buffer (no offset): nothing is remembered at all
    assert a.forms.get(None, a.w, 0, _Desc(4, 8, 3), 0, 0, None, "sp", a.single) == "single" and len(fs.used) == 1


@pytest.mark.parametrize("other", [{"c_out": 16}, {"c0": 8}, {"ci_first": 2}, {"n_in": 2}, {"mode": 1}, {"lift": True}, {"off": 4},
                                   {"engine": "nhwc"}])
def test_another_descriptor_column_range_mode_or_lift_flag_is_another_form(fake_packset, other):
    a = _Asker()
    a.forward(1)
    a.get()
    a.forward(2)
    assert a.get() is fake_packset.built[0].buffers[0] and a.singles == 1
    assert a.get(**other) == "single" and a.singles == 2
    a.forward(3)
    assert sum(a.forms.sizes().values()) == 2
    assert a.get(**other) is not a.get() and a.singles == 2


def test_switched_off_there_are_no_sets_and_nothing_is_queued(fake_packset):
    a = _Asker(enabled=False)
    for g in range(1, 4):
        a.forward(g)
        assert a.get() == "single" and a.get(engine="nhwc") == "single"
    assert a.singles == 6 and a.forms.sizes() == {} and a.forms._engines == {} and fake_packset.built == []
