"""CPU tests of the pair kernels' planner (pair_choose in pair_sweeps.h, behind dafs_hipk_pairhmm_plan and
dafs_hipk_pairhmm5_plan): the instances it knows are the ones pair_instances.TABLES states, and every plan it returns is
one the launch accepts.  The launch's conditions are restated here (pair_instances.fits); no launch function is called.
Without a device the planner works from the occupancies the instances were compiled for, on a GPU machine from the
code objects' register counts: the assertions hold for either."""
import pytest

import pair_instances as pi

NTASKS = (1, 100, 1000, 4200, 5000, 9000, 20000, 200000)
MAX_LEN1 = (100, 500, 959, 960, 1000, 1500, 1919, 1920, 2047, 3839, 3840)
MAX_LEN2 = (1, 10, 30, 60, 100, 127, 200, 223, 255, 400, 511, 1000, 1023, 1024, 2047, 2048)
ETOOLONG = -4


@pytest.mark.parametrize("model", [0, 1])
def test_the_compiled_instances_are_the_stated_ones(model):
    assert pi.discover(model) == pi.TABLES[model]


def test_the_limits_follow_from_the_tables():
    """what README.md states: rows at most 3839, columns at most 2047 (ProbCons) and 1023 (CONTRAlign)"""
    assert max(pi.ROW_LIMIT.values()) == 3839
    assert [max(g * w for g, w in pi.TABLES[m]) - 1 for m in (0, 1)] == [2047, 1023]


@pytest.mark.parametrize("model", [0, 1])
def test_every_plan_launches(model):
    """Nothing forced.  A plan that is returned names an instance whose lanes hold max_len2 + 1 columns and whose row
    pointers (4 wavefronts x 64/G groups x (max_len1 + 1) words) fit the 60 KiB the launch allows; DAFS_HIP_ETOOLONG is
    returned exactly when no instance of the table satisfies both.  Every case of the grid is looked at before the test
    fails, and the failure lists them."""
    from dafs_amd import capi
    plan = capi.PairhmmPlan()
    bad = []
    with pi.forced(None, None):
        for ntasks in NTASKS:
            for l1 in MAX_LEN1:
                for l2 in MAX_LEN2:
                    rc = pi.plan_fn(model)(ntasks, l1, l2, plan)
                    possible = any(pi.fits(g, w, l1, l2) for g, w in pi.TABLES[model])
                    assert possible == (l1 <= 3839 and l2 <= (1023 if model else 2047))
                    if rc == 0:
                        g, w = plan.group, plan.width
                        ok = ((g, w) in pi.TABLES[model] and g * w >= l2 + 1 and plan.slab_steps == l1 + g
                              and 4 * (64 // g) * (plan.slab_steps - g + 1) * 4 <= 60 * 1024 and possible)
                        if not ok:
                            bad.append((ntasks, l1, l2, "plan (%d, %d), slab_steps %d" % (g, w, plan.slab_steps)))
                    elif rc != ETOOLONG or possible:
                        bad.append((ntasks, l1, l2, "rc %d, an instance fits: %s" % (rc, possible)))
    assert not bad, "%d of %d plans: %s" % (len(bad), len(NTASKS) * len(MAX_LEN1) * len(MAX_LEN2), bad[:12])


@pytest.mark.parametrize("model", [0, 1])
def test_forcing_filters_before_the_row_limit(model):
    """A forced group whose row pointers the launch would refuse leaves nothing: DAFS_HIP_ETOOLONG, not another group."""
    from dafs_amd import capi
    plan = capi.PairhmmPlan()
    for g, limit in pi.ROW_LIMIT.items():
        w = pi.widths(model, g)[0]
        with pi.forced(g, w):
            assert pi.plan_fn(model)(1, limit, g * w - 1, plan) == 0
            assert (plan.group, plan.width, plan.slab_steps) == (g, w, limit + g)
            assert pi.plan_fn(model)(1, limit + 1, g * w - 1, plan) == ETOOLONG
            assert pi.plan_fn(model)(1, limit, g * w, plan) == ETOOLONG
        with pi.forced(g, None):
            assert pi.plan_fn(model)(1, limit, 10, plan) == 0 and plan.group == g
            assert pi.plan_fn(model)(1, limit + 1, 10, plan) == ETOOLONG
