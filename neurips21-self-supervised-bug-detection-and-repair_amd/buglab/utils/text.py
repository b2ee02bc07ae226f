"""Cutting a snippet's text at code ranges -- the contract of reference buglab/utils/text.py:12-84 (`get_text_in_range`,
`text_to_range_segments`) and of `relative_range` (buglab/utils/cstutils.py:46-61), on plain tuples: a position is
`(line, column)`, a range `((line, column), (line, column))`, end exclusive.  Lines count from 1 and end at "\\n" only (the
reference reads them from an `io.StringIO`); columns count from 0.  Nothing here needs libcst."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Sequence, Tuple

Position = Tuple[int, int]
Range = Tuple[Position, Position]


def as_range(r) -> Range:
    """A range as stored in a datapoint (nested lists after msgpack) -> hashable tuples."""
    return ((r[0][0], r[0][1]), (r[1][0], r[1][1]))


def split_lines(text: str) -> List[str]:
    """The lines `io.StringIO(text).readline()` returns: cut after every "\\n", nowhere else."""
    parts = text.split("\n")
    lines = [p + "\n" for p in parts[:-1]]
    if parts[-1]:
        lines.append(parts[-1])
    return lines


def _slice(line: str, start, end) -> str:
    stop = None if end is None or end == math.inf else end
    return line[(0 if start is None else start):stop]


def text_of_lines(lines: Sequence[str], rng) -> str:
    (l0, c0), (l1, c1) = rng
    out = []
    first = max(int(l0), 1)
    last = len(lines) if l1 == math.inf else min(int(l1), len(lines))
    for line_no in range(first, last + 1):
        line = lines[line_no - 1]
        if l0 == l1:
            out.append(_slice(line, c0, c1))
        elif line_no == l0:
            out.append(_slice(line, c0, None))
        elif line_no == l1:
            out.append(_slice(line, None, c1))
        else:
            out.append(line)
    return "".join(out)


def get_text_in_range(text: str, rng) -> str:
    """The text between two positions.  A start line of 0 (before the text) and an end of (inf, inf) are allowed."""
    return text_of_lines(split_lines(text), rng)


def relative_range(base: Range, target: Range) -> Range:
    """`target` as positions inside the text that `base` covers: lines from 1; columns shifted on the first line only."""
    (bl, bc), (el, ec) = base
    (sl, sc), (tl, tc) = target
    if (sl, sc) < (bl, bc) or (tl, tc) > (el, ec):
        raise ValueError(f"range {target} is not inside {base}")
    rel_start_line = sl - bl + 1
    rel_end_line = rel_start_line + tl - sl
    return ((rel_start_line, sc - bc if rel_start_line == 1 else sc), (rel_end_line, tc - bc if rel_end_line == 1 else tc))


def non_empty(rng: Range) -> Range:
    """An empty range is widened by one column, so that it has something to mark."""
    start, end = rng
    return (start, (end[0], end[1] + 1)) if start == end else rng


def shown_ranges(segment_range: Range, target_ranges: Iterable[Range]) -> Dict[Range, Range]:
    """{widened relative range: target range}.  Two targets that become the same relative range collide: the later one is
    kept (the reference builds this dict the same way)."""
    return {non_empty(relative_range(segment_range, t)): t for t in target_ranges}


def text_to_range_segments(text_segment: str, segment_range, target_ranges: Iterable) -> List[Tuple[str, List[Range]]]:
    """`text_segment` (which covers `segment_range`) cut at every start and end of the target ranges: [(text, the target ranges
    that cover it)], in text order; the texts concatenate to `text_segment`.  Within a segment the ranges are listed by
    (start, end) -- the reference has a set there."""
    relative = shown_ranges(as_range(segment_range), [as_range(t) for t in target_ranges])
    at_point: Dict[Position, List[Range]] = {}
    for r in relative:
        at_point.setdefault(r[0], []).append(r)
        at_point.setdefault(r[1], []).append(r)
    lines = split_lines(text_segment)
    active: Dict[Range, None] = {}
    out: List[Tuple[str, List[Range]]] = []
    current: Tuple = (0, 0)
    for point in sorted(at_point):
        out.append((text_of_lines(lines, (current, point)), sorted(relative[r] for r in active)))
        for r in at_point[point]:  # a range opens at its start and closes at its end
            if r in active:
                del active[r]
            else:
                active[r] = None
        current = point
    assert not active
    out.append((text_of_lines(lines, (current, (math.inf, math.inf))), []))
    return out
