"""The settings contract of the item-weight models in one place (no GPU): what `implicit` and `dense_output` do to the
cached lists, the readiness and the weights of CooccurrenceModel, EASEModel, SLIMModel and SimilarityAggregation, all of it
the shared layer of polara_amd/models.py (_ItemWeightModel)."""
import numpy as np
import pytest

MODELS = {   # name: (the attributes that hold its weights, dense_output by default, what a changed `implicit` does)
    'CooccurrenceModel': (('_i2i',), False, 'renews'),
    'EASEModel': (('_weights', 'precision_diagonal'), True, 'renews'),
    'SLIMModel': (('_W', 'sweeps'), True, 'renews'),
    'SimilarityAggregation': (('_S', '_St'), False, 'refreshes'),
}


class _NoDevice:
    """stands where the device backend would: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError('the device backend was touched (%s)' % name)


@pytest.mark.parametrize('name', sorted(MODELS))
def test_settings_contract(name):
    import polara_amd
    from polara_amd.data import ArrayData
    slots, dense_default, implicit_change = MODELS[name]
    u, i, v = np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0])
    m = getattr(polara_amd, name)(ArrayData((u, i, v), n_users=2, n_items=2), ops=_NoDevice())
    assert m.implicit is False and m.dense_output is dense_default
    assert all(getattr(m, slot) is None for slot in slots)

    def arm():
        m._is_ready, m._recommendations = True, object()
        for slot in slots:
            setattr(m, slot, object())

    def state():
        """(ready, lists kept, weights kept)"""
        held = [getattr(m, slot) is not None for slot in slots]
        assert all(held) or not any(held)
        return m._is_ready, m._recommendations is not None, held[0]
    kept, refreshed, renewed = (True, True, True), (True, False, True), (False, False, False)

    arm()
    m.implicit, m.dense_output = False, dense_default          # equal values: nothing happens
    assert state() == kept
    m.implicit = True
    assert m.implicit is True and state() == (renewed if implicit_change == 'renews' else refreshed)
    arm()
    if name == 'EASEModel':                                     # fixed at True
        with pytest.raises(NotImplementedError, match='dense_output is fixed at True'):
            m.dense_output = False
        assert m.dense_output is True and state() == kept
    else:
        m.dense_output = not dense_default                      # the other branch: new lists, the same model
        assert m.dense_output is (not dense_default) and state() == refreshed
    arm()
    m._renew_model()
    assert state() == renewed
