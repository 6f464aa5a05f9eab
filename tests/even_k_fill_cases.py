"""Gap lists whose true paths run THROUGH palindromic k-mers (even k), shared by tests/test_even_k_fill_cases.py (the
oracle alone, no GPU) and tests/test_gpu_even_k_fill.py (every fill path against the oracle).

A palindromic k-mer has one strand: the node that spells the reverse complement of v is v itself, not v ^ 1, and
pred(v) = succ(v ^ 1) ^ 1 fails at it and at each of its successors (tests/even_k_cases.py has the graph's rules).  Every
class below is an island of its own — a random sequence around a planted palindrome, a read by itself — with gaps cut
across it so that the palindrome lies on the path that fills the gap:

  a  in the middle of a non-branching stretch
  b  the left flank's last k-mer (the deepest left seed), with and without fuz
  c  the right flank's first k-mer (right seed rmf), a later right seed (0 < j < rmf), and the only one (rmf = 0)
  d  next to a bubble of a second haplotype: a SNP one base in front of the palindrome (the palindrome has two parents),
     on its first base (its successor has two parents, one of them the palindrome) and one base behind it
  e  two palindromes in a row: a stretch of period 4 (ACGT...) and one of period 2 (AT...)
  f  a tandem array whose unit holds a palindrome: the k-mer at several depths
  g  a hairpin (s + revcomp(s)): both strands of every k-mer of s on one path.  The oracle does NOT flag it: the walk
     through the centre meets the two strands of a k-mer at different depths, and Q7 is both strands in ONE border.  The
     Q7 cases of these lists are class d's gaps over the substitution on the palindrome's first base, where the
     palindrome and its one-base neighbour lead into each other's strands at one depth; class_condition asserts that
     the oracle flags some gap, so that the rule "what the oracle flags carries G2S_GAP_Q7" is exercised next to a
     palindrome

K lists the k the cases are made for: the first width of each k-mer word at which the islands do not merge."""
import cases
import even_k_cases
import pyref

K = (12, 32, 64)
D_ERR = 100
FUZ = 10
CLASSES = "abcdef"


def _cut(cls, island, pos, end, k, lmf, rmf, pal):
    """the gap [pos, end) of island, flanks of k + fuz bases on either side"""
    assert pos - k - lmf >= 0 and end + k + rmf <= len(island) and end > pos
    return dict(cls=cls, pal=pal, left=island[pos - k - lmf:pos], right=island[end:end + k + rmf], gap_len=end - pos + k,
                lmf=lmf, rmf=rmf, true_len=end - pos)


def _other(c, by=1):
    return "ACGT"[("ACGT".index(c) + by) & 3]


def build(k):
    """(reads, gaps): gaps are cut_gaps-style dicts with two more keys, cls (the class's letter) and pal (the palindrome
    planted on the gap's path)"""
    assert k % 2 == 0
    rng = cases.SplitMix(9100 + k)
    pad = k + FUZ + 24  # a flank with full fuz and some room inside the gap
    reads, gaps = [], []

    def rand(n):
        return cases.random_dna(rng, n)

    # a: X + P + Y, the gap from inside X to inside Y
    for _ in range(2):
        x, p = rand(pad + 10), even_k_cases.palindrome(rng, k)
        isl = x + p + even_k_cases._not_mirrored(x, rand(pad + 10))
        reads.append(isl)
        gaps.append(_cut("a", isl, k + FUZ + 4, len(isl) - k - FUZ - 4, k, FUZ, FUZ, p))
        gaps.append(_cut("a", isl, k + 9, len(isl) - k - 7, k, 3, 0, p))
    # b: the left flank ends with P
    x, p = rand(pad), even_k_cases.palindrome(rng, k)
    isl = x + p + even_k_cases._not_mirrored(x, rand(2 * pad + 30))
    reads.append(isl)
    for lmf in (FUZ, 1, 0):
        gaps.append(_cut("b", isl, len(x) + k, len(isl) - k - FUZ - 3, k, lmf, FUZ, p))
    # c: the right flank starts with P, or holds it a few bases in
    x, p = rand(2 * pad + 30), even_k_cases.palindrome(rng, k)
    isl = x + p + even_k_cases._not_mirrored(x, rand(pad))
    reads.append(isl)
    for rmf, back in ((FUZ, 0), (FUZ, 4), (FUZ, FUZ), (0, 0), (5, 2)):
        gaps.append(_cut("c", isl, k + FUZ + 3, len(x) - back, k, FUZ, rmf, p))
    # d: a second haplotype with one substitution next to P
    for where in (-1, 0, k):
        x, p = rand(pad + 20), even_k_cases.palindrome(rng, k)
        isl = x + p + even_k_cases._not_mirrored(x, rand(pad + 20))
        at = len(x) + where
        hap = isl[:at] + _other(isl[at], 2 if where == 0 else 1) + isl[at + 1:]  # (where == 0: not P's other half's mirror)
        reads += [isl, hap]
        gaps.append(_cut("d", isl, k + FUZ + 2, len(isl) - k - FUZ - 2, k, FUZ, FUZ, p))
        gaps.append(_cut("d", isl, k + 5, len(isl) - k - 6, k, 2, 3, p))
    # e: stretches of period 4 and period 2 between two random contexts
    for unit in ("ACGT", "AT"):
        x, y = rand(pad + 8), rand(pad + 8)
        mid = unit * ((k + 8) // len(unit) + 1)
        isl = x + mid + y
        reads.append(isl)
        pals = [mid[i:i + k] for i in range(len(mid) - k + 1) if mid[i:i + k] == pyref.revcomp(mid[i:i + k])]
        assert len(set(pals)) == 2
        gaps.append(_cut("e", isl, k + FUZ + 3, len(isl) - k - FUZ - 3, k, FUZ, FUZ, pals[0]))
        gaps.append(_cut("e", isl, k + 6, len(isl) - k - 4, k, 0, 2, pals[0]))
    # f: a tandem array of four units, P + 17 bases each
    x, y, p = rand(pad + 6), rand(pad + 6), even_k_cases.palindrome(rng, k)
    isl = x + (p + rand(17)) * 4 + y
    reads.append(isl)
    gaps.append(_cut("f", isl, k + FUZ + 2, len(isl) - k - FUZ - 2, k, FUZ, FUZ, p))
    gaps.append(_cut("f", isl, k + 7, len(isl) - k - 5, k, 4, 1, p))
    # g: a hairpin; the gap runs through its centre, from s into revcomp(s)
    s = rand(2 * pad)
    isl = s + pyref.revcomp(s)
    reads.append(isl)
    gaps.append(_cut("g", isl, k + FUZ + 5, len(isl) - k - FUZ - 5, k, FUZ, FUZ, s[len(s) - k // 2:] + pyref.revcomp(s)[:k // 2]))
    return reads, gaps


def padded(k, total=264):
    """(reads, gaps): build(k) beside a toy genome, the list filled up with gaps cut from it to `total` gaps (just over
    the 256 at which a list runs resident by default); the added gaps have cls None"""
    reads, gaps = build(k)
    toy = cases.toy_genome(k + 1, 12000, k, repeats=8, tandem=2, snp_every=500)
    more = cases.cut_gaps(k + 1, toy[0], k, FUZ, total - len(gaps), 40, 200, D_ERR)
    for g in more:
        g["cls"], g["pal"] = None, None
    return reads + toy, gaps + more


def on_path(g, fill):
    """the planted palindrome lies in the filled sequence, read with the flank ends around it"""
    k = len(g["pal"])
    text = (g["left"][-(k + g["lmf"]):] + fill + g["right"][:k + g["rmf"]]).upper()
    return g["pal"] in text


def class_condition(gaps, outcomes):
    """outcomes[i] = (count, q7, fill, draws) of gap i by the oracle.  Asserts, class by class, that a..f each have a gap
    the oracle fills without a Q7 flag through the planted palindrome, that class d has one with a choice to draw at
    (several paths), that the hairpin gap of class g is filled through its centre and not flagged either, and that some
    gap of the list is a Q7 case.  Returns {class: [indices of its good gaps]}."""
    good = {c: [] for c in CLASSES + "g"}
    for i, (g, (count, q7, fill, draws)) in enumerate(zip(gaps, outcomes)):
        if g["cls"] in good and count > 0 and not q7 and on_path(g, fill):
            good[g["cls"]].append(i)
    for c in CLASSES:
        assert good[c], "class %s: no gap that the oracle fills through its palindrome without Q7" % c
    # (g is no Q7 case, see above: then it is a gap that is filled through the hairpin's centre and compared like the rest)
    assert good["g"], "class g: the oracle does not fill the hairpin gap through its centre, or flags it"
    assert any(outcomes[i][0] >= 2 and outcomes[i][3] > 1 for i in good["d"]), "class d: no gap whose traceback has a choice"
    assert any(o[1] for g, o in zip(gaps, outcomes) if g["cls"]), "no designed gap is a Q7 case"
    return good
