"""The tick engine's list and ring rules ("The lists' rules") in plain Python integers: what an evaluation's
items are and where they stand in a slot's block, which evaluations go to the chain area, how long a reservation is, how
tick_reserve_kernel shares waiting problems among the segments' free slots.  Workgroups append to a list in an order nobody fixes, so
nothing here predicts WHERE a block stands: check_list decodes a returned list and checks everything the rules do fix."""
from _gn_f64 import pts_per_thread

THREADS = 256
NOOP, CAND, CHUNK_BITS, SENTINEL = 0x80000000, 0x40000000, 12, 0x3FFFF5A5
MAX_SEGS = 20
ST_IDLE, ST_RUNNING, ST_GOOD, ST_ABORTED, ST_BAD_AFFINE = range(5)
# the point counts at which one of the two chunk tables changes its points per thread: the last n under the smaller figure
TABLE_EDGES = (256, 512, 1024, 2048, 4 * 1024 - 1, 16 * 1024 - 1, 64 * 1024 - 1, 256 * 1024 - 1)


def chunks_of(n, ppt):
    return -(-n // (THREADS * ppt))


def num_chunks(n, geometry):
    return chunks_of(n, pts_per_thread(n, geometry))


def max_chunks_upto(cap):
    """the largest chunk count any n <= cap has under any of the three tables: under one figure of points per thread the count grows
    with n, so only cap itself and the last n before a table moves on can hold the maximum"""
    return max(num_chunks(n, g) for g in (0, 1, 2) for n in (cap,) + TABLE_EDGES if n <= cap)


def npos(nch):
    """list positions of an evaluation of nch chunks: its chunks, from eight chunks on rounded up to whole rounds of the eight XCDs"""
    return nch if nch < 8 else 8 * -(-nch // 8)


def position_chunk(nch, p):
    """the chunk at position p of an evaluation's positions, None for a no-op.  Position p runs on XCD p mod 8 (relative to the block's
    start); XCD x takes the band of ceil(nch / 8) consecutive chunks from x * ceil(nch / 8) on, one per round p // 8"""
    if nch < 8:
        return p
    per_xcd = -(-nch // 8)
    chunk = (p & 7) * per_xcd + (p >> 3)
    return chunk if chunk < nch else None


def item(slot, chunk, cand):
    return (slot << CHUNK_BITS) | chunk | (CAND if cand else 0)


def decode(word):
    """('noop',) | ('sentinel',) | ('item', slot, chunk, cand)"""
    if word == SENTINEL:
        return ("sentinel",)
    if word & NOOP:
        return ("noop",)
    return ("item", (word & ~(NOOP | CAND)) >> CHUNK_BITS, word & ((1 << CHUNK_BITS) - 1), bool(word & CAND))


def block(slot, nch, twin, length=None):
    """the words of a slot's block: the main candidate's positions, behind them the twin's with the candidate bit, then no-ops up to
    `length` (a reservation longer than what was used)"""
    words = []
    for cand in ((False, True) if twin else (False,)):
        for p in range(npos(nch)):
            c = position_chunk(nch, p)
            words.append(NOOP if c is None else item(slot, c, cand))
    assert length is None or length >= len(words)
    return words + [NOOP] * ((length or 0) - len(words))


def chain_eligible(chain_cap, chain_max_n0, nch, twin, n0):
    return chain_cap > 0 and nch == 1 and not twin and (chain_max_n0 <= 0 or n0 <= chain_max_n0)


def reservation(chain_cap, chain_max_n0, nch, want_twin, n0):
    """words a step reserves early for its next evaluation of nch chunks (0: none -- the chain area takes it, or an empty level)"""
    if chain_eligible(chain_cap, chain_max_n0, nch, want_twin, n0):
        return 0
    return (2 if want_twin else 1) * npos(nch)


def staged(chain_cap, chain_max_n0, nch, twin, n0, reserved=0):
    """what staging an evaluation adds: (chain entry?, block length, words of an abandoned reservation).  A reservation that holds the
    evaluation is used and padded; a shorter one is turned into no-ops and a fresh block follows"""
    if chain_eligible(chain_cap, chain_max_n0, nch, twin, n0):
        return True, 0, reserved
    total = (2 if twin else 1) * npos(nch)
    if total == 0:  # an empty level: nothing to evaluate, a reservation (there is none for an empty level) would be left as no-ops
        return False, 0, reserved
    if total > reserved:
        return False, total, reserved
    return False, reserved, 0


# ---- tick_reserve_kernel ----------------------------------------------------------------------------------------------------------
def shares(nfree, avail):
    """entries each segment of one kind takes: all its free slots where enough problems wait, else the floor of its proportional
    share, the remainder one each from the first segment on where a free slot is left"""
    total = sum(nfree)
    if total <= avail:
        return list(nfree)
    take = [avail * f // total for f in nfree]
    left = avail - sum(take)
    for i, f in enumerate(nfree):
        if left > 0 and take[i] < f:
            take[i] += 1
            left -= 1
    return take


def rank_index(base, rank):
    return base + rank


def reserve(segs, running, head, count):
    """(admit_idx per slot, heads afterwards): -2 where no segment covers a slot, -1 for a running slot or one that gets nothing"""
    idx = [-2] * len(running)
    heads = list(head)
    for mode in (0, 1):
        mine = [s for s in segs if s[0] == mode]
        nfree = [sum(1 for j in range(i0, i0 + ns) if not running[j]) for _, i0, ns in mine]
        take = shares(nfree, max(count[mode] - head[mode], 0))
        base = head[mode]
        for (_, i0, ns), tk in zip(mine, take):
            rank = 0
            for j in range(i0, i0 + ns):
                if running[j]:
                    idx[j] = -1
                else:
                    idx[j] = rank_index(base, rank) if rank < tk else -1
                    rank += 1
            base += tk
        heads[mode] = base
    return idx, heads


# ---- a returned list ----------------------------------------------------------------------------------------------------------------
def check_list(items, cap, chain_cap, count0, chain0, count, chain, blocks, chains, abandoned=0, overflowed=False, preplaced=()):
    """items: the whole allocation (cap item slots, chain_cap chain entries, the guard region).  blocks: {slot: (nch, twin, length)} of
    the slots whose evaluation became items; chains: the slots that became chain entries; abandoned: words of reservations turned into
    no-ops (those the count grew by).  preplaced: slots whose block stands in words the caller reserved below count0.  count / chain:
    the counters read back.  overflowed: the list ran over -- blocks may be cut at cap, the chain area holds
    chain_cap distinct eligible slots; nothing at or behind cap is an item or a no-op either way."""
    items = [int(w) for w in items]
    want_count = count0 + sum(b[2] for s, b in blocks.items() if s not in preplaced) + abandoned
    assert count == want_count, ("count", count, want_count)
    assert chain == chain0 + len(chains), ("chain", chain, chain0 + len(chains))
    assert overflowed == (count > cap or chain > chain_cap), ("overflow", count, cap, chain, chain_cap)
    end = min(count, cap)
    covered = [False] * end
    starts = {}
    for i in range(0, end):
        d = decode(items[i])
        if d[0] == "item" and d[2] == 0 and not d[3]:
            assert d[1] not in starts, ("slot staged twice", d[1], starts[d[1]], i)
            starts[d[1]] = i
    for slot, (nch, twin, length) in blocks.items():
        if slot not in starts:
            assert overflowed, ("slot's block is missing", slot)
            continue
        s = starts[slot]
        want = block(slot, nch, twin, length)
        assert overflowed or s + len(want) <= end, ("block runs past the count", slot, s, len(want), end)
        got = items[s:min(s + len(want), end)]
        assert got == want[:len(got)], ("block", slot, nch, twin, s, [hex(w) for w in got[:20]], [hex(w) for w in want[:20]])
        for i in range(s, s + len(got)):
            assert not covered[i], ("blocks overlap", slot, i)
            covered[i] = True
    assert set(starts) <= set(blocks), ("items of a slot that staged none", sorted(set(starts) - set(blocks)))
    for i in range(0, end):
        if not covered[i]:
            assert items[i] == NOOP or (i < count0 and items[i] == SENTINEL), ("stray word", i, hex(items[i]))
    assert all(w == SENTINEL for w in items[end:cap]), ("written behind the count", [(i, hex(items[i])) for i in range(end, cap) if items[i] != SENTINEL][:5])
    assert all(w == SENTINEL for w in items[cap:cap + chain0]), "the chain entries that were there"
    in_chain = items[cap + chain0:cap + min(chain, chain_cap)]
    assert len(set(in_chain)) == len(in_chain) and set(in_chain) <= set(chains), ("chain entries", in_chain[:10], sorted(chains)[:10])
    assert overflowed or set(in_chain) == set(chains)
    assert all(w == SENTINEL for w in items[cap + min(chain, chain_cap):cap + chain_cap]), "the unused chain entries"
    guard = items[cap + chain_cap:]
    assert all(w == SENTINEL for w in guard), ("guard region", [(cap + chain_cap + i, hex(w)) for i, w in enumerate(guard) if w != SENTINEL][:5])


def build_list(cap, chain_cap, chain_max_n0, count0, slots, guard=64):
    """a list as slots staging one after the other, in the order given, would leave it (an order among the many the device may take):
    slots = [(slot, nch, twin, n0, reserved)].  Returns (items, count, chain, blocks, chains, abandoned) for check_list"""
    items = [SENTINEL] * (cap + chain_cap + guard)
    count, chain, blocks, chains, abandoned = count0, 0, {}, [], 0
    reserved_at = {}
    for slot, nch, twin, n0, reserved in slots:  # the reservations are made first (early in the step)
        reserved_at[slot] = count
        count += reserved
    for slot, nch, twin, n0, reserved in slots:
        to_chain, length, dropped = staged(chain_cap, chain_max_n0, nch, twin, n0, reserved)
        base = reserved_at[slot]
        if dropped:
            items[base:base + dropped] = [NOOP] * dropped
            abandoned += dropped
        if to_chain:
            items[cap + chain] = slot
            chain += 1
            chains.append(slot)
            continue
        if length == 0:
            continue
        if dropped or not reserved:
            base = count
            count += length
        items[base:base + length] = block(slot, nch, twin, length)
        blocks[slot] = (nch, twin, length)
    return items, count, chain, blocks, chains, abandoned
