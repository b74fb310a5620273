"""runtime.HandleOwner, the base of PerceptualLoss, VGGParameterNet, ParameterPredictor, EndToEndTrainer and
StrategyClassifier, against a device stand-in that counts: no GPU."""
import gc

import pytest

from underwater_image_enhancement_amd.runtime import HandleOwner


class FakeDevice:
    def __init__(self, index):
        self.index = index
        self.created, self.destroyed = [], []
        self.fail_destroy = False

    def create(self, *key):
        self.created.append(key)
        return ("handle", self.index, key, len(self.created))

    def destroy(self, handle):
        if self.fail_destroy:
            raise RuntimeError("the device is gone")
        self.destroyed.append(handle)


class Owner(HandleOwner):
    def _create_handle(self, dev, *key):
        return dev.create(*key)

    @staticmethod
    def _destroy_handle(dev, handle):
        dev.destroy(handle)


def test_one_handle_per_key_and_close_frees_each_once():
    a, b = FakeDevice(0), FakeDevice(1)
    owner = Owner()
    h = owner._handle(a)
    assert owner._handle(a) is h and a.created == [()]  # created once
    hp = owner._handle(a, 1)  # a further key on the same GPU (PerceptualLoss: the precision)
    assert hp is not h and owner._handle(a, 1) is hp and a.created == [(), (1,)]
    hb = owner._handle(b)
    assert b.created == [()] and len(owner._handles) == 3
    owner.close()
    assert sorted(a.destroyed, key=str) == sorted([h, hp], key=str) and b.destroyed == [hb]
    assert len(owner._handles) == 0
    owner.close()  # nothing left to free
    assert len(a.destroyed) == 2 and len(b.destroyed) == 1


def test_close_before_any_use_and_use_after_close():
    a = FakeDevice(0)
    owner = Owner()
    owner.close()
    assert a.created == [] and a.destroyed == []
    h1 = owner._handle(a)
    owner.close()
    h2 = owner._handle(a)  # created again
    assert h2 != h1 and a.created == [(), ()] and a.destroyed == [h1]
    owner.close()
    assert a.destroyed == [h1, h2]


def test_del_closes_and_swallows_a_failing_destroy():
    a = FakeDevice(0)
    owner = Owner()
    h = owner._handle(a)
    del owner
    gc.collect()
    assert a.destroyed == [h]
    owner = Owner()
    owner._handle(a)
    a.fail_destroy = True
    with pytest.raises(RuntimeError, match="the device is gone"):
        owner.close()  # close() itself reports it
    owner._handle(a)
    owner.__del__()  # what the interpreter runs at collection: no exception leaves it
    del owner
    gc.collect()
