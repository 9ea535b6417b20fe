"""Reference stepper for life-like rules (helper of the rule tests, not a test): a numpy torus
stepper that sums the eight np.rolls of the board and looks the sum up in the two masks.

A rule is (birth, survive), two 9-bit masks: birth bit n = a dead cell with exactly n alive
neighbours of its 8 becomes alive, survive bit n = an alive cell with exactly n stays alive.
Boards are uint8 arrays of 0/1 here; to_bytes / from_bytes convert to the library's 0/255.
"""
import numpy as np

CONWAY = (0x008, 0x00C)


def masks(text: str) -> tuple[int, int]:
    """Canonical "B<digits>/S<digits>" -> (birth, survive).  (The library's own parser is under
    test; this one only reads well-formed rules written in the tests.)"""
    b, s = text.split("/")
    assert b[0] == "B" and s[0] == "S", text
    return sum(1 << int(d) for d in b[1:]), sum(1 << int(d) for d in s[1:])


def neighbours(board: np.ndarray) -> np.ndarray:
    n = np.zeros(board.shape, dtype=np.uint8)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                n += np.roll(np.roll(board, dy, axis=0), dx, axis=1)
    return n


def step(board: np.ndarray, birth: int, survive: int) -> np.ndarray:
    n = neighbours(board)
    blut = np.array([(birth >> i) & 1 for i in range(9)], dtype=np.uint8)
    slut = np.array([(survive >> i) & 1 for i in range(9)], dtype=np.uint8)
    return np.where(board != 0, slut[n], blut[n]).astype(np.uint8)


def run(board: np.ndarray, rule, turns: int, keep=()):
    """`turns` turns of `rule` (text or mask pair).  Returns (final board, counts after every
    turn, {t: board after t turns for t in keep})."""
    birth, survive = masks(rule) if isinstance(rule, str) else rule
    b = (np.asarray(board) != 0).astype(np.uint8)
    counts, kept = [], {}
    if 0 in keep:
        kept[0] = b
    for t in range(1, turns + 1):
        b = step(b, birth, survive)
        counts.append(int(b.sum()))
        if t in keep:
            kept[t] = b
    return b, counts, kept


def random_board(seed: int, H: int, W: int, density: float) -> np.ndarray:
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def to_bytes(board: np.ndarray) -> np.ndarray:
    return (np.asarray(board) != 0).astype(np.uint8) * 255


def from_bytes(world: np.ndarray) -> np.ndarray:
    return (np.asarray(world) == 255).astype(np.uint8)
