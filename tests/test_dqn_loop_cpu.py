"""workers.cut_updates: how TrainDeviceDQN(updates_per_graph > 0) cuts the updates of one run() into ddrl_dqn_loop_run calls — maximal
runs of one (node, buffer), ended by every update whose number is a multiple of push_freq (the weights go out behind it).  Hand-written
cases; REFERENCE: the per-update loop of algos/dqn/train.py:213-231 (`if cnt % push_freq == 0: push`, then `cnt += 1`) replayed here."""
import numpy as np

from distributed_drl_amd.workers import cut_updates

A, B, C = (0, 0), (0, 1), (1, 0)


def _per_update(choices, cnt, push_freq):
    """The reference's loop, one update at a time: [(key, update number, pushes behind it)]."""
    return [(key, cnt + i, (cnt + i) % push_freq == 0) for i, key in enumerate(choices)]


def _expand(pieces, cnt):
    out = []
    for key, k, push in pieces:
        assert k >= 1
        for j in range(k):
            out.append((key, cnt, push and j == k - 1))
            cnt += 1
    return out


def test_one_buffer_between_pushes_is_one_call():
    assert cut_updates([A] * 7, 1, 300) == [(A, 7, False)]
    assert cut_updates([], 1, 300) == []
    assert cut_updates([A], 299, 300) == [(A, 1, False)]


def test_a_push_ends_its_piece():
    # updates 48 .. 53, push behind update 50
    assert cut_updates([A] * 6, 48, 50) == [(A, 3, True), (A, 3, False)]
    # the run ends on the push
    assert cut_updates([A] * 3, 48, 50) == [(A, 3, True)]
    # two pushes inside one run
    assert cut_updates([A] * 9, 3, 4) == [(A, 2, True), (A, 4, True), (A, 3, False)]


def test_a_push_on_the_first_update():
    assert cut_updates([A] * 4, 50, 50) == [(A, 1, True), (A, 3, False)]
    assert cut_updates([A], 100, 50) == [(A, 1, True)]


def test_push_freq_one_cuts_every_update():
    assert cut_updates([A, A, B], 1, 1) == [(A, 1, True), (A, 1, True), (B, 1, True)]


def test_buffer_changes_cut_and_equal_neighbours_merge():
    ch = [A, A, B, B, B, A, C, C]
    assert cut_updates(ch, 1, 300) == [(A, 2, False), (B, 3, False), (A, 1, False), (C, 2, False)]
    # a buffer change and a push on the same update; the same buffer on both sides of a push stays cut
    assert cut_updates([A, A, B, B, B], 9, 10) == [(A, 2, True), (B, 3, False)]
    assert cut_updates([A, B, B, B], 9, 10) == [(A, 1, False), (B, 1, True), (B, 2, False)]


def test_pieces_replay_the_per_update_loop():
    rs = np.random.RandomState(4)
    for push_freq in (1, 2, 5, 7, 300):
        for cnt in (1, 4, 5, 6, 299, 300):
            ch = [(int(rs.choice(2, 1)[0]), int(rs.choice(3, 1)[0])) for _ in range(41)]
            pieces = cut_updates(ch, cnt, push_freq)
            assert _expand(pieces, cnt) == _per_update(ch, cnt, push_freq)
            for (k0, _, p0), (k1, _, _) in zip(pieces, pieces[1:]):
                assert p0 or k0 != k1, "two neighbouring pieces that one call could have run"
