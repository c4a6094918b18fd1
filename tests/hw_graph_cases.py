"""Candidate sets of tests/test_gpu_hw_window_graph.py (plain data makers, no GPU): the five cuts of one sequence, random families of cut
and substituted roots, the medium set."""
import random


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def five_cuts():
    """One 300-base sequence whole and cut four ways: with ignore_ends_len 15 three edges hold in one direction only, and the row of
    the whole sequence ends with two entries the symmetrisation appends."""
    s = rnd(random.Random(8), 300)
    return {"whole": s, "a": s[13:-13], "b": s[20:], "c": s[:-26], "d": s[5:-5]}


def family(seed, n=40, roots=3, lo=150, hi=300, cut=30, subs=3):
    """About n sequences: 0..cut bases off either end of one of `roots` random sequences of lo..hi bases, 0..subs substitutions."""
    rng = random.Random(seed)
    base = [rnd(rng, rng.randint(lo, hi)) for _ in range(roots)]
    C = {}
    for i in range(n):
        s = base[i % roots]
        s = list(s[rng.randint(0, cut):len(s) - rng.randint(0, cut)])
        for _ in range(rng.randint(0, subs)):
            p = rng.randrange(len(s))
            s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
        C["f%d_%d" % (seed, i)] = "".join(s)
    return C


def medium(seed=77, n=600, roots=3, length=700):
    """About 600 sequences in three families of about 700 bases: well above 2 048 window pairs."""
    return family(seed, n=n, roots=roots, lo=length - 20, hi=length + 20, cut=30, subs=3)


def sorted_list(C):
    """The list get_NN_graph_ignored_ends_edlib aligns: unique sequences (last accession wins), stable sort by length."""
    return sorted({seq: acc for acc, seq in C.items()}.items(), key=lambda x: len(x[0]))
