"""CPU: the numpy restatement of the octree path keys (tests/octree_ref.py) against hand-computed keys and against the
CPU oracle's octree (oracle/sph_oracle_grav.c, which recurses like the reference), and the properties the adversarial
particle sets of tests/test_octree_adversarial_gpu.py are built to have."""
import numpy as np
import pytest

import octree_ref as R

ALL7 = (1 << 63) - 1                     # child 7 at every one of the 21 levels


def key_of(*children):
    """key whose first levels are `children` and whose remaining levels are all child 7"""
    k = 0
    for ch in children:
        k = (k << 3) | ch
    rest = R.LEVELS - len(children)
    return (k << (3 * rest)) | ((1 << (3 * rest)) - 1)


def test_hand_computed_keys_in_the_unit_cube():
    # the unit cube's corners fix the root box: centre 0.5, edge 1
    x = np.array([0.0, 1.0, 0.5, 0.75, 0.25])
    y = np.array([0.0, 1.0, 0.5, 0.25, 1.0])
    z = np.array([0.0, 1.0, 0.5, 0.5, 0.0])
    k = R.path_keys(x, y, z)
    assert int(k[0]) == 0                                   # the low corner: child 0 all the way down
    assert int(k[1]) == ALL7                                # the high corner: child 7 all the way down
    # the root centre lies on all three split planes: low child at level 0, then above every later centre
    assert int(k[2]) == key_of(0)
    # (0.75, 0.25, 0.5): level 0 -> x high only (1); level 1 centre (0.75, 0.25, 0.25): x and y on the plane -> low,
    # z high (4); level 2 centre (0.625, 0.125, 0.375): all high from there on
    assert int(k[3]) == key_of(1, 4)
    # (0.25, 1, 0): level 0 -> y high (2); level 1 centre (0.25, 0.75, 0.25): x on the plane -> low, y high, z low (2);
    # then x stays above every later centre (0.125, 0.1875, ...), y high, z = 0 low: 1 | 2 = 3 for the other 19 levels
    assert int(k[4]) == key_of(2, 2, *([3] * 19))
    assert int(k[4]) == _slow_key(0.25, 1.0, 0.0, (0.5, 0.5, 0.5), 1.0)


def _slow_key(px, py, pz, c, size):
    """one particle, plain Python floats, the reference's recursion written out"""
    c = list(c)
    key = 0
    for _ in range(R.LEVELS):
        b = [px > c[0], py > c[1], pz > c[2]]
        key = (key << 3) | (int(b[0]) | int(b[1]) << 1 | int(b[2]) << 2)
        q = 0.25 * size
        c = [c[a] + (q if b[a] else -q) for a in range(3)]
        size *= 0.5
    return key


def test_points_on_a_split_plane_go_to_the_low_child():
    # a lattice whose root edge is a power of two: points on the level-0 plane x = 32 share the low child with x < 32
    g = R.lattice(k=33, spacing=2.0)
    k = R.path_keys(g["x"], g["y"], g["z"])
    top = (k >> np.uint64(60)).astype(np.int64)
    on = g["x"] == 32.0
    assert on.sum() == 33 * 33
    assert np.all(top[on] & 1 == 0) and np.all(top[g["x"] > 32.0] & 1 == 1)
    # every lattice point against the scalar restatement
    rng = np.random.default_rng(0)
    c, s = R.root_box(g["x"], g["y"], g["z"])
    for i in rng.choice(g["x"].size, 200, replace=False):
        assert int(k[i]) == _slow_key(g["x"][i], g["y"][i], g["z"][i], c, s)
    # a '>=' rule would give different keys for every point on any split plane
    assert np.unique(k).size == g["x"].size


@pytest.mark.parametrize("name", ["lattice33", "sheet", "line", "plummer", "sparse_cube", "two_clusters", "ragged257"])
def test_key_octree_has_the_oracle_octrees_node_count(name):
    """the octree the keys describe (a node splits while it holds more than one particle) has as many nodes as the
    oracle's explicit octree of the same particles, built by the reference's recursion"""
    from oracle import orc_grav
    g = R.FAMILIES[name]()
    k = R.path_keys(g["x"], g["y"], g["z"])
    assert np.unique(k).size == k.size                        # no two keys coincide in these sets
    t = orc_grav.Tree(g["x"], g["y"], g["z"], g["m"])
    assert R.octree_node_count(k) == orc_grav.lib().orcg_tree_nodes(t.h)
    t.free()


def test_shared_keys_family_has_the_coinciding_keys_it_promises():
    g = R.shared_keys()
    k = R.path_keys(g["x"], g["y"], g["z"])
    c, s = R.root_box(g["x"], g["y"], g["z"])
    assert s < 0.025 * 2.0 ** R.LEVELS                     # soft^2 = 0.0025 accepts every node of edge < 0.025
    n0 = 3000
    # every planted twin shares its partner's key, the triple shares one key three ways, and the first particle of each
    # straddling pair shares the key of the cloud particle whose box it was planted in: 39 + 8 pairs, one triple
    uk, cnt = np.unique(k, return_counts=True)
    assert np.sum(cnt == 2) == 39 + 8 and np.sum(cnt == 3) == 1 and np.sum(cnt > 3) == 0
    assert np.unique(k[:n0]).size == n0                    # the cloud itself: all distinct
    twins = k[n0:n0 + 40]
    assert np.all(np.isin(twins, k[:n0]))
    # the straddling pairs: closer than a level-21 edge, but in neighbouring boxes
    a, b = k[n0 + 41:n0 + 49], k[n0 + 49:n0 + 57]
    assert np.all(a != b) and np.all(R.common_levels(a, b) < R.LEVELS)
    assert np.all(np.abs(g["x"][n0 + 41:n0 + 49] - g["x"][n0 + 49:n0 + 57]) < s / 2.0 ** R.LEVELS)


def test_common_levels_and_degenerate_boxes():
    assert R.common_levels(np.uint64(0), np.uint64(1)) == 20
    assert R.common_levels(np.uint64(0), np.uint64(1 << 60)) == 0
    assert R.common_levels(np.uint64(ALL7), np.uint64(ALL7 - (1 << 30))) == 10
    # all coincident: root edge 0, every key 0
    g = R.coincident()
    c, s = R.root_box(g["x"], g["y"], g["z"])
    assert s == 0.0 and np.all(R.path_keys(g["x"], g["y"], g["z"]) == 0)
    # flat sheet: z = 0 lies ON the root's z plane (low child), then above every later centre (high child)
    g = R.sheet()
    k = R.path_keys(g["x"], g["y"], g["z"])
    zmask = np.uint64(int("100" * 21, 2))
    assert np.all(k & zmask == zmask & np.uint64(ALL7 >> 3))
    # a line along x: the same for y and z
    g = R.line()
    k = R.path_keys(g["x"], g["y"], g["z"])
    yzmask = np.uint64(int("110" * 21, 2))
    assert np.all(k & yzmask == yzmask & np.uint64(ALL7 >> 3))


def test_families_fit_the_budget():
    for name, f in R.FAMILIES.items():
        g = f()
        assert 1 <= g["x"].size <= 200_000, name
        assert np.all(g["u"] == 0.0) and np.all(g["vx"] == 0.0) and np.all(g["alpha"] == 0.0), name
        h = R.own_h(g)
        assert h.shape == g["x"].shape and np.all((h >= 0.05) & (h <= 10.0)), name
