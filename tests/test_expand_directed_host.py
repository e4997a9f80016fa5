"""tetris_hip_expand_envs against the oracle on the directed boards, on CPU (harness backend): the per-env body
expand_kernel runs, on the instantiation the library picks for the geometry, and the host logic of expand_from / expand
/ two_ply_values (tests/expand_directed_cases.py has the cases, the geometry list and the coverage conditions).

What the oracle produced (60 near-top boards at every geometry) -- run entries / entries of dst; run entries that clear
1, 2, 3, 4 lines; children over under their dictated piece; parents over of the source batch; rescued placements:

    5x20    6727 /  9004   810 139 29 18   449  127 of 1153  53      6x20    8130 / 10638   806 111 27 21   469  125 of 1179  72
    7x20    9553 / 12296   734 110 30 24   466  160 of 1207  73      8x20   11253 / 14269   771 112 35 27   489  142 of 1233  64
    9x20   12587 / 15825   803 111 36 30   473  157 of 1261  61      10x20  14044 / 17521   806 112 39 33   505  162 of 1287  72
    10x10  13775 / 17182   783 115 40 33   489  150 of 1261  60      10x13  13968 / 17434   786 112 41 33   442  188 of 1287  89
    6x4     4194 /  5862   561  84 32  9   453  150 of  937  89      10x4    6352 /  8452   607 110 42 13   498  158 of 1045  68
    11x20  15941 / 19720   813 117 42 36   416  150 of 1315  60      12x20  17300 / 21304   794 127 45 39   429  185 of 1341  84
    10x24  13808 / 17251   826 114 39 33   397  193 of 1287  95      11x27  16050 / 19844   793 120 42 36   437  175 of 1315  65
    10x40  13764 / 17201   786 115 39 33   410  184 of 1287  89      9x40   11998 / 15152   797 110 36 30   462  173 of 1261  98
    12x40  17761 / 21830   820 123 45 39   456  159 of 1341  63      10x32  13997 / 17467   787 114 39 33   492  154 of 1287  65
    10x33  13513 / 16914   754 111 39 33   519  185 of 1287  76      10x44  14169 / 17665   826 113 39 33   401  176 of 1287  80
    10x45  14623 / 18182   813 112 39 33   390  170 of 1287  82      12x59  18144 / 22268   793 125 45 39   443  166 of 1341  53
    10x21  14451 / 17986   793 116 39 33   432  150 of 1287  82      10x28  14188 / 17685   713 121 39 33   418  175 of 1287  63
    10x56  13549 / 16955   783 115 39 33   479  181 of 1287  84      10x57  13861 / 17312   810 112 39 33   445  167 of 1287  85
    5x59    6541 /  8792   807 127 30 18   480  143 of 1153  54

Every floor of expand_directed_cases.FLOORS holds at every geometry; none is lowered."""
import pytest

import expand_cases as ec
import expand_directed_cases as ed

DEV = "cpu"
KEYS = sorted(ed.bk.KEY_CASES)


def test_geometry_list(host_backend):
    ed.geometry_list(DEV)


@pytest.mark.parametrize("C,R", ed.EXPAND_GEOMETRIES)
def test_two_generations(host_backend, orc, C, R):
    ed.two_generations(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", ed.DIRECTION_GEOMETRIES)
def test_feature_directions(host_backend, orc, C, R):
    ed.feature_directions(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", ed.DRAWN_GEOMETRIES)
def test_drawn_same_for_every_child(host_backend, orc, C, R):
    ed.drawn_same_for_every_child(DEV, orc, C, R)


@pytest.mark.parametrize("name", KEYS)
def test_drawn_at_key_edges(host_backend, orc, name):
    ed.drawn_at_key_edges(DEV, orc, name)


@pytest.mark.parametrize("C,R,n", ed.SET_SIZE_CASES)
def test_bag_set_sizes(host_backend, orc, C, R, n):
    ed.bag_set_sizes(DEV, orc, C, R, n)


@pytest.mark.parametrize("C,R", ed.TWO_PLY_GEOMETRIES)
def test_two_ply_vs_oracle(host_backend, orc, C, R):
    ec.two_ply_vs_oracle(DEV, orc, C, R)
