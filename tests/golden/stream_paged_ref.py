"""Reference for the PAGED streaming caches (M2FNet.stream(pages=...), csrc/attention_stream.hip's paged form): the addressing, in plain
float64 torch, and nothing else.

A `PagedSite` keeps the K / V rows of one attention site for many slots in two pools [n_pages, page_rows, E].  Logical cache row r of a
slot - utterance r of a plain cache, utterance u with u % C == r of a ring of C rows - is row r % page_rows of page
table[slot][r // page_rows].  `attend` gathers the slot's live rows through the table in utterance order, hands them to the rule of
tests/golden/stream_ref.py (`_Site.attend`: append the new row, keep the last past + 1, softmax(q K^T / sqrt(hd)) V), and stores the
new row at its place.  Fed the same histories it must give exactly what a `stream_ref._Site` per slot gives, whatever the table looks
like; tests/test_stream_paged_cpu.py holds it to that.  The pools start as NaN, so a row gathered from the wrong place shows.
"""
from __future__ import annotations

from typing import List, Sequence

import torch
from torch import Tensor

import stream_ref


def position(n_old: int, capacity: int, ring: bool) -> int:
    """the logical cache row utterance n_old takes"""
    return n_old % capacity if ring else n_old


def live_rows(n_old: int, capacity: int, ring: bool) -> List[int]:
    """logical cache rows of the utterances cached so far, oldest first (a ring: the last `capacity` of them)"""
    first = max(0, n_old - capacity) if ring else 0
    return [position(u, capacity, ring) for u in range(first, n_old)]


def address(table_row: Sequence[int], r: int, page_rows: int):
    """(page, row inside the page) of logical cache row r"""
    return int(table_row[r // page_rows]), r % page_rows


class PagedSite:
    def __init__(self, n_pages: int, page_rows: int, capacity: int, ring: bool, E: int):
        self.R, self.C, self.ring = page_rows, capacity, ring
        self.kpool = torch.full((n_pages, page_rows, E), float("nan"), dtype=torch.float64)
        self.vpool = torch.full((n_pages, page_rows, E), float("nan"), dtype=torch.float64)

    def gather(self, pool: Tensor, table_row: Sequence[int], n_old: int) -> List[Tensor]:
        return [pool[address(table_row, r, self.R)] for r in live_rows(n_old, self.C, self.ring)]

    def attend(self, q: Tensor, k: Tensor, v: Tensor, n_head: int, table_row: Sequence[int], n_old: int) -> Tensor:
        """The slot's new rows q, k, v [E] against the n_old utterances it has cached; stores k / v; returns [E]."""
        site = stream_ref._Site(self.C - 1 if self.ring else None)
        site.k, site.v = self.gather(self.kpool, table_row, n_old), self.gather(self.vpool, table_row, n_old)
        out = site.attend(q.double(), k.double(), v.double(), n_head)
        page, row = address(table_row, position(n_old, self.C, self.ring), self.R)
        self.kpool[page, row], self.vpool[page, row] = k.double(), v.double()
        return out
