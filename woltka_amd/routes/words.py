"""Packed records accumulated per sample (wk_words_*): the weighted histogram
for plain ranks (csrc/wk_weigh.hpp) and the per-read stream for `--rank free`
/ `--uniq` / `--above` / `--major` (csrc/wk_free.hpp), both over one
accumulation for a set that mixes the two kinds; which job sets they take."""
import os

import numpy as np

from .. import _native as nat
from ..hostio import MAX_GROUPS, ROUTES


def whole_reads(job):
    """Does the job look at whole reads?  `--rank free`, a rank under --uniq /
    --above / --major above one half: the per-read stream (csrc/wk_free.hpp).
    Never a size-normalised job."""
    if job.flags & nat.F_SIZED:
        return False
    if job.mode == nat.MODE_FREE:
        return True
    return job.mode == nat.MODE_RANK and (
        job.major > 0.5 or (job.major <= 0 and bool(
            job.flags & (nat.F_UNIQ | nat.F_ABOVE))))


def plain_job_ok(job):
    """Is the job one the weighted histogram takes (csrc/wk_weigh.hpp)?"""
    if job.flags & nat.F_UNIQ:
        return False
    if job.mode == nat.MODE_RANK and (job.flags & nat.F_ABOVE or
                                      job.major > 0):
        return False
    return job.mode in (nat.MODE_NONE, nat.MODE_RANK)


def list_job(job):
    """Can the job split a read over several features, so that its read map
    holds a list?  none without --uniq, a rank without --uniq / --above /
    --major (classify.py:32-51, 81-127)."""
    if job.flags & nat.F_UNIQ:
        return False
    if job.mode == nat.MODE_NONE:
        return True
    return job.mode == nat.MODE_RANK and not job.flags & nat.F_ABOVE and \
        job.major <= 0


class WordsRoute:
    """(mixin of classify.Engine)"""

    def words_mixed(self):
        """Does the job set hold whole-read jobs next to other jobs?  Such a
        set goes through ``wk_words_begin_mixed`` (`_words_begin`)."""
        n = sum(map(whole_reads, self.jobs))
        return 0 < n < len(self.jobs)

    def _words_begin(self, group):
        """The job set declared for the records that follow: through the
        mixed entry when the set is mixed (``WOLTKA_NO_MIXED=1``: never)."""
        return self.ctx.words_begin(self.jobs, group, mixed=self._mixed_on())

    def _mixed_on(self):
        return self.words_mixed() and not os.environ.get('WOLTKA_NO_MIXED')

    def _count_mixed(self):
        """A block or chunk appended under a mixed set (`ROUTES['mixed']`)."""
        if self._mixed_on():
            ROUTES['mixed'] += 1

    def words_eligible(self, identity=True, sized=False, mixed=False):
        """Can chunks go to the device as packed words, accumulated per
        sample (``wk_words_*``)?  The plain assigners only — what
        ``wk_words_begin`` checks once more against the subject table.
        ``identity``: the words come from the host tokenizer, whose ids must
        be the subject indices (the device text route translates).
        ``sized``: the caller can take `--sizes` this way (`sized_on_device`:
        plain classification of a whole file); then a set of plain
        size-normalised jobs is eligible too — its flush makes the rows of
        the contribution log (csrc/wk_sized.hpp, `_collect_sized`).  Sized
        jobs that look at whole reads keep the general route.
        ``mixed``: the caller declares the set through ``_words_begin``; then
        whole-read jobs next to plain ones, none of them sized, are eligible
        too (``WOLTKA_NO_MIXED=1``: not)."""
        if (self.sizes and not sized) or self._replay is not None or \
                len(self.jobs) > nat.MAX_JOBS or \
                (identity and not self._tok_identity) or \
                os.environ.get('WOLTKA_NO_WORDS'):
            return False
        # jobs that look at whole reads — `--rank free`, a rank under --uniq /
        # --above / --major above one half — all go to the per-read stream
        # (csrc/wk_free.hpp), alone or several of them
        if all(map(whole_reads, self.jobs)):
            return self.use_tree
        if mixed and self._mixed_on():
            # (the plain jobs of the set: what the histogram takes, unsized)
            return bool(self.use_tree) and all(
                plain_job_ok(job) and not job.flags & nat.F_SIZED
                for job in self.jobs if not whole_reads(job))
        return all(map(plain_job_ok, self.jobs))

    @staticmethod
    def sized_on_device(plain, part=None):
        """Does `--sizes` keep the words route for this file?  Plain
        classification only (``plain``: no `--outmap`, `--outcov`, `--demux`,
        `--stratify`, `--coords`) of a whole file (``part``: a byte range of
        a file keeps today's route).  ``WOLTKA_NO_DSIZES=1`` keeps every
        `--sizes` call on the general route."""
        return bool(plain and part is None and
                    not os.environ.get('WOLTKA_NO_DSIZES'))

    def device_maps_eligible(self):
        """Can the read maps be formatted on the device (wk_readmap.hpp)?  The
        plain assigners, i.e. the job sets the weighted histogram takes."""
        if self.sizes or self._replay is not None or \
                len(self.jobs) > nat.MAX_JOBS or not self._tok_identity or \
                os.environ.get('WOLTKA_NO_WORDS') or \
                os.environ.get('WOLTKA_NO_DMAPS'):
            return False
        for job in self.jobs:
            if job.flags & (nat.F_UNIQ | nat.F_SIZED | nat.F_ABOVE) or \
                    job.major > 0 or \
                    job.mode not in (nat.MODE_NONE, nat.MODE_RANK):
                return False
        return True

    def read_maps_on_device(self, fmt, demux=False, strata=False,
                            coords=False, outcov=False, part=None,
                            own_text=True):
        """Can the read maps of this file be formatted on the device from the
        assignment codes (csrc/wk_readmap_reads.hpp, `_run_dreads_maps`)?
        Plain classification with `--outmap` of a whole file (``part``) of
        SAM, BLAST tabular, PAF or simple-map text that can be read block by
        block (``own_text``: a plain file or a gzip file this package inflates
        itself), with or without `--trim-sub` / `--exclude`, when no job of the
        set can return a list: every job is `--rank free`, a rank under --uniq
        / --above / --major, or none under --uniq (`whole_reads`, or none with
        --uniq).  Not under ``demux``, ``strata``, ``coords``, ``outcov`` or
        `--sizes`, not during the replay pass, not with more than `MAX_JOBS`
        jobs.  A set that holds a job able to return a list keeps today's
        routes (plain jobs only: `device_maps_eligible`).
        ``WOLTKA_NO_DREADMAPS=1`` (like ``WOLTKA_NO_DTOK=1``) keeps the
        general route."""
        if os.environ.get('WOLTKA_NO_DREADMAPS') or \
                os.environ.get('WOLTKA_NO_DTOK'):
            return False
        if demux or strata or coords or outcov or self.sizes or \
                self._replay is not None or part is not None or \
                not own_text or fmt not in ('sam', 'b6o', 'paf', 'map') or \
                not 1 <= len(self.jobs) <= nat.MAX_JOBS:
            return False
        for job in self.jobs:
            if job.flags & nat.F_SIZED:
                return False
            if job.mode == nat.MODE_NONE:
                if not job.flags & nat.F_UNIQ:
                    return False
            elif not (whole_reads(job) or (job.mode == nat.MODE_RANK and
                                           job.major > 0)):
                return False
        return True

    def read_map_lists_on_device(self, fmt, demux=False, strata=False,
                                 coords=False, outcov=False, part=None,
                                 own_text=True):
        """Can the read maps of this file be formatted on the device when a
        job of the set can return a list (csrc/wk_readmap_lists.hpp,
        `_run_dreads_lists`)?  Asked where neither `device_maps_eligible` nor
        `read_maps_on_device` took the file.  The scope of
        `read_maps_on_device` -- plain classification with `--outmap` of a
        whole file of SAM, BLAST tabular, PAF or simple-map text read block by
        block, with or without `--trim-sub` / `--exclude`; not under
        ``demux``, ``strata``, ``coords``, ``outcov`` or `--sizes`, not during
        the replay pass, 1 to `MAX_JOBS` jobs, none size-normalised -- for the
        sets that hold at least one job able to split a read: none without
        --uniq, or a plain rank without --uniq / --above / --major
        (`list_job`).  The other jobs of the set may be of any kind.
        ``WOLTKA_NO_DLISTMAPS=1`` (like ``WOLTKA_NO_DTOK=1``) keeps the
        general route."""
        if os.environ.get('WOLTKA_NO_DLISTMAPS') or \
                os.environ.get('WOLTKA_NO_DTOK'):
            return False
        if demux or strata or coords or outcov or self.sizes or \
                self._replay is not None or part is not None or \
                not own_text or fmt not in ('sam', 'b6o', 'paf', 'map') or \
                not 1 <= len(self.jobs) <= nat.MAX_JOBS:
            return False
        if any(job.flags & nat.F_SIZED for job in self.jobs):
            return False
        return any(map(list_job, self.jobs))

    def demux_read_maps_on_device(self, fmt, demux=True, strata=False,
                                  coords=False, outcov=False, part=None,
                                  own_text=True):
        """Can the read maps of this file be formatted on the device although
        the file is demultiplexed (csrc/wk_readmap_demux.hpp,
        `_run_dreads_demux`)?  Plain classification with `--outmap` of a file
        that is demultiplexed (``demux``: `--demux`, or a single-file input):
        the whole file (``part``) of SAM, BLAST tabular, PAF or simple-map
        text that can be read block by block (``own_text``: a plain file or a
        gzip file this package inflates itself), with or without `--trim-sub`
        / `--exclude`, `--samples`, `--unassigned`, `--name-as-id`; 1 to
        `MAX_JOBS` jobs of any kind, none size-normalised (a set with a job
        able to return a list is formatted by the list formatter, every other
        set by the formatter of whole-read assignments).  Not under
        ``strata``, ``coords``, ``outcov`` or `--sizes`, not during the replay
        pass.  ``WOLTKA_NO_DDEMUXMAPS=1`` (like ``WOLTKA_NO_DDEMUX=1`` and
        ``WOLTKA_NO_DTOK=1``) keeps the host route."""
        if os.environ.get('WOLTKA_NO_DDEMUXMAPS') or \
                os.environ.get('WOLTKA_NO_DDEMUX') or \
                os.environ.get('WOLTKA_NO_DTOK'):
            return False
        if not demux or strata or coords or outcov or self.sizes or \
                self._replay is not None or part is not None or \
                not own_text or fmt not in ('sam', 'b6o', 'paf', 'map') or \
                not 1 <= len(self.jobs) <= nat.MAX_JOBS:
            return False
        return not any(job.flags & nat.F_SIZED for job in self.jobs)

    def _run_words(self, data, packed, sample):
        """One chunk of packed records (``('words', array, n_reads, slot)``
        from `native_chunks`): appended to the sample's records on the device,
        which are classified by one launch when the sample ends
        (``wk_words_flush`` — any fetch of the counts flushes)."""
        _, words, n, slot = packed
        ring = self._ring
        if (sample, None) not in self.group_ids:
            # a new sample: room for its group id and for the keys it can add
            # (one per job and taxon, at most one per subject) — checked once
            # per sample, not per chunk: looking at the table waits for the
            # device
            if len(self.groups) + 1 >= MAX_GROUPS // 2:
                self.collect(data)
            self._ensure_table(data, max(len(self.subjects), 1 << 16) + 1, 1)
        group = self._group_array(n, sample, None)
        for rank in self.ranks:
            data[rank].setdefault(sample, {})
        self._n_reads += n
        known = len(self.subj_feature)
        if len(self.subjects) > known:
            self.subj_feature.extend(self.index.intern_many(
                self.subjects.names[known:]))
            self.ctx.set_subjects(self.subj_feature)
            # (a key per job and subject at most; the table is never left to
            # fill up)
            if 4 * len(self.subjects) * len(self.jobs) > self.slots_reserved \
                    and not self._table_fixed:
                self.collect(data, keep_groups=True)
                self._reserve(8 * len(self.subjects) * len(self.jobs))
        if self.sizes:      # (rows of the samples flushed so far, once many)
            self._collect_sized(force=False)
        if self._words_begin(group):
            self.ctx.words_append(words, n, slot)
            self._count_mixed()
            # the buffer of the chunk before this one has been copied by now
            if self._ring_prev is not None:
                self.ctx.words_wait(self._ring_prev)
                ring.release(self._ring_prev)
            self._ring_prev = slot
            return n
        # the general route (a subject without an ancestor at some rank):
        # subject indices and read offsets out of the words
        w = np.array(words)                 # (off the pinned buffer)
        ring.release(slot)
        subj = (w & np.uint32((1 << nat.Context.WORD_SUBJ_BITS) - 1)
                ).astype(np.int32)
        starts = np.flatnonzero((w >> np.uint32(nat.Context.WORD_POS_SHIFT)) &
                                np.uint32(15) == 0)
        qoff = np.concatenate((starts, [w.size])).astype(np.int32)
        self.ctx.chunk_stage(subj, qoff, group=group, subj_is_set=True,
                             indexed=True)
        self._classify_staged(data, False)
        if self.sizes:
            self._collect_log()
        return n

    def _words_done(self):
        """The last staging buffer in flight goes back to the ring."""
        if self._ring_prev is not None:
            self.ctx.words_wait(self._ring_prev)
            self._ring.release(self._ring_prev)
            self._ring_prev = None
