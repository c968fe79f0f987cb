"""CPU: the plan of tests/test_gpu_mixed_step3.py -- its sequence, its conditions and its orders -- without a device.

The GPU module asserts, from the plain-Python planners, that its sequence is what it is there for (enough ring ops and volume entry points;
msf_pyramid regrown across the 2-D / 3-D boundary; s3_coef needs of several sizes whose two largest belong to different families) and that
every order it issues keeps every op after the ops it names.  Nothing of that needs a GPU: here the sequence is built over addresses that
are never used (DryMem), every condition and every order is checked, and the float64 models confirm the input condition of msssim3f_model's
bounds on the pairs the GPU module holds to them.
"""
import msssim3f_model as M3
import msssimf_model as MS
import test_gpu_mixed_step3 as T


def test_the_sequence_meets_its_conditions_and_every_order_is_admissible():
    seq = T.Sequence3(T.DryMem(), None)                          # build() asserts conditions()
    assert len(seq.ops) == 40
    T.conditions(seq, say=True)
    orders = T.planned_orders(seq)                               # asserts check_order, the trims and the two halves
    for how in ("ascending", "descending"):
        T.pyramid_walk(orders[how][0], how)
    for title in sorted(orders):
        T.show(title, orders[title][0])
    seq.free()


def test_the_multi_scale_pairs_keep_every_weighted_mean_away_from_zero():
    """msssim3f_model's bounds hold where every m_s with a weight is at least 0.2: pair 0 of both groups, in float64."""
    seq = T.Sequence3(T.DryMem(), None)
    for name in ("ms3.vol", "ms3.big"):
        op = seq.by_name[name]
        scales, weights = op.config
        wts = MS.check_weights(scales, weights)
        means = M3.Model(op.pairs[0][0], op.pairs[0][1], T.RANGE).means(scales)
        low = min(float(means[s][1] if s == scales - 1 else means[s][0]) for s in range(scales) if wts[s] > 0)
        print("%s: lowest weighted m_s %.3f" % (name, low))
        assert low >= T.MIN_MEAN, (name, low)
    seq.free()
