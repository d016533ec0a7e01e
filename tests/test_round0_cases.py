"""CPU tests of the generators behind the round-0 GPU tests (round0_cases.py): exact sizes, the skip cap of the
adversarial seeds with the oracle alone, and the restated symbol code against the properties the cases rely on."""
import numpy as np

import oracle_lib as O
import round0_cases as R


def test_sized_text_is_exact():
    _, words = R.edge_vocab(7)
    for length, nb, end in ((5000, 700, None), (5000, 4999, None), (5000, 5000, None), (5000, 0, None), (4097, 3, "blank"),
                            (4097, 2000, "letter"), (4097, 4000, "blank")):
        text = R.sized_text(length, words, length, nb, end=end)
        assert len(text) == length and R.kept(text) == length - nb + 1 and R.n_symbols(text) == length + 1
        if end and 0 < nb < length:
            assert (chr(text[-1]) in R.BLANKS) == (end == "blank")


def test_adversarial_skip_cap():
    """At most one of eight seeds of the adversarial group may be refused by the oracle (vocabulary construction), and
    every kind and flavour is among those that run."""
    seeds = list(range(24))  # test_gpu_round0_edges.C_SEEDS (that module needs the GPU library's package; not imported here)
    ran = []
    for seed in seeds:
        _, vocab, kind, flavour = R.big_case(seed, with_text=False)
        try:
            O.Vocab(vocab)
            ran.append((kind, flavour))
        except O.OracleError:
            pass
    assert len(seeds) - len(ran) <= len(seeds) // 8
    assert {k for k, _ in ran} == set(R.BIG_KINDS) and {f for _, f in ran} == set(R.BIG_FLAVOURS)


def test_code_model_is_alphabetic_and_complete():
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 200, 256):
        lens = R.garsia_wachs([float(x) for x in rng.integers(1, 10000, size=n)])
        assert abs(sum(2.0 ** -l for l in lens) - 1.0) < 1e-9  # a full binary tree
    # only an end of the alphabet can take one bit
    assert R.garsia_wachs([1.0, 100.0, 1.0])[1] == 2 and R.garsia_wachs([1.0, 1.0, 100.0])[2] == 1
