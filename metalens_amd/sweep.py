"""Batched source sweeps with the sums kept on the GPU.

The reference's docstring describes the use (nearfield.py:69-73): an isotropic or Lambertian
emitter is the INCOHERENT sum of x-, y- and z-polarised dipoles, possibly at several positions -
i.e. many runs of near field -> far field whose POWERS are added, and whose efficiency is
``sum(total_P) / sum(power_passing_through_lens)`` (nearfield_farfield.py:74, nearfield.py:474-477).

What a sweep shares:

* tables, layout, far-field plan and the per-sample geometry records (ring, sector, rotated
  coordinates, nearest cell: csrc/nearfield_geometry.hip) - they depend on grid and lens only;
* within a group of sources at ONE position that differ in polarisation (the x, y, z triple): the
  whole per-sample evaluation except the two weights the incident H enters with - such a group
  is ONE synthesis pass (``ml_nearfield_batch_async``) that leaves one resident field set per
  member;
* the sums: ``P_sum``, per-source ``total_P`` and encircled power are accumulated by a kernel
  right after each projection (``ml_farfield_accumulate``); only ``P_sum`` and two scalars per
  source cross PCIe, whatever the sweep's length;
* with ``image=`` (a ``PlanePropagator``): the image of the emitter at finite distance.  The field sets of a
  group are propagated to the image plane in ONE pass (``ml_propagate_sets``: the geometry of a (sample, target)
  pair serves all members) and their weighted ``|E|^2`` and ``Sz`` are summed on the GPU
  (``ml_propagate_accumulate``); two real maps cross PCIe at the end.  With ``image_radii=`` the sums are reduced
  further on the GPU (``ml_propagate_focus``): peak, moments and the power inside each radius, and from it the focusing
  efficiency ``encircled power / incident power``.
"""
import numpy as np

from . import _lib, constants, packing, ties
from .grating import n_glass as tabulated_n_glass
from .nearfield import _check_axis, _raise_violation, nearfield_params
from .pipeline import _check_source
from .postprocess import BEAM_RECORD, _beam_dict, _beam_single, _check_beam

MAX_BATCH = 3          # members of a polarisation batch (csrc/nearfield_dev.h MAX_POL)
MAX_SLOTS = 4096       # ML_MAX_SWEEP_SLOTS


class SourceSweep:
    def __init__(self, wavelength, lens_periphery_summary, lens_center_summary, hexgridset,
                 x_pts, y_pts, ux, uy, dipole_moment=None, c0=None, Z0=None, ctx=None,
                 precision=None, method=None, units=None):
        self.ctx = ctx or _lib.default_context()
        # context-wide settings, re-asserted by every prepare() (other objects share the context)
        self.precision = precision or 'f64'
        self.method = method or 'auto'
        self.owner = _lib.new_owner()
        self.ctx.set_precision(self.precision)
        self.ctx.set_method(self.method)
        self.units = constants.as_units(units)   # the caller's unit system (nearfield.build_nearfield); default SI
        self.c0 = self.units.c0 if c0 is None else c0
        self.Z0 = self.units.Z0 if Z0 is None else Z0
        if dipole_moment is None:
            dipole_moment = constants.default_dipole_moment(self.units)
        _check_axis(x_pts, wavelength)
        _check_axis(y_pts, wavelength)
        S = lens_periphery_summary
        wl_nm = int(round(wavelength / self.units.nm))
        n_glass = S['gratingcollection_list'][0].grating_list[0].n_glass
        if n_glass == 0:
            n_glass = tabulated_n_glass(wl_nm)
        self.n_glass, self.wavelength = n_glass, wavelength
        self._tables = (S['gratingcollection_list'], hexgridset, wl_nm)
        self._layout = (S, lens_center_summary)
        self._cells = lens_center_summary
        self.dipole_moment = dipole_moment
        self.x, self.y = _lib.f64(x_pts), _lib.f64(y_pts)
        self.ux, self.uy = _lib.f64(np.ravel(ux)), _lib.f64(np.ravel(uy))
        self.dxp, self.dyp = x_pts[1] - x_pts[0], y_pts[1] - y_pts[0]

    def prepare(self, check_content=True):
        """make tables, layout and the far-field plan resident (no-ops when they already are).
        ``check_content=False`` (``queue``): trust the content hashes of the last full ``prepare``
        as long as the context still holds the tables and layout it left there - hashing the
        caller's 30 MB of cells on every queued pass would make a sweep host-bound"""
        ctx, lib = self.ctx, self.ctx.lib
        mine = getattr(self, '_resident', None)
        if check_content or mine is None or mine != (ctx.tables_token, ctx.layout_token):
            packing.upload_tables(ctx, *self._tables)
            packing.upload_layout(ctx, *self._layout)
            self._resident = (ctx.tables_token, ctx.layout_token)
        ctx.set_precision(self.precision)
        ctx.set_method(self.method)
        _lib.check(lib.ml_nearfield_premodulate(ctx.handle, 0))
        _lib.check(lib.ml_farfield_plan(ctx.handle, self.x.size, self.y.size, self.dxp, self.dyp,
                                        self.wavelength, self.n_glass, _lib.dptr(self.ux),
                                        self.ux.size, _lib.dptr(self.uy), self.uy.size, 0))
        ctx.plan_owner = ctx.fields_owner = self.owner

    def _check_image(self, image):
        """argument errors of ``image=``, before any device call"""
        if image is None:
            return
        if image.ctx is not self.ctx:
            raise ValueError('image= must be a PlanePropagator built on the context of this sweep (ctx=sweep.ctx)')
        if tuple(image.aperture_shape) != (self.x.size, self.y.size):
            raise ValueError('image= was built for an aperture of %d x %d samples, the sweep\'s grid has %d x %d'
                             % (tuple(image.aperture_shape) + (self.x.size, self.y.size)))

    def _check_pupil(self, pupil):
        """argument errors of ``pupil=``, before any device call"""
        if pupil is None:
            return
        if pupil.ctx is not self.ctx:
            raise ValueError('pupil= must be an AperturePupil built on the context of this sweep (ctx=sweep.ctx)')
        if tuple(pupil.shape) != (self.x.size, self.y.size):
            raise ValueError('pupil= was built for an aperture of %d x %d samples, the sweep\'s grid has %d x %d'
                             % (tuple(pupil.shape) + (self.x.size, self.y.size)))

    def _check_zone_fields(self, zone_fields):
        """argument errors of ``zone_fields=``, before any device call"""
        if zone_fields is None:
            return
        if zone_fields.ctx is not self.ctx:
            raise ValueError('zone_fields= must be an ApertureZoneFields built on the context of this sweep (ctx=sweep.ctx)')
        if tuple(zone_fields.shape) != (self.x.size, self.y.size):
            raise ValueError('zone_fields= was built for an aperture of %d x %d samples, the sweep\'s grid has %d x %d'
                             % (tuple(zone_fields.shape) + (self.x.size, self.y.size)))

    def queue(self, sources, image=None, beam_cones=None, beam_centre='peak', pupil=None):
        """queue the whole sweep on the GPU and return without synchronising (benchmarks);
        tie settlement and the downloads are ``run``'s business.

        NOT content-checked: ``queue`` trusts the hashes taken by the last ``prepare()`` / ``run()``
        of this object.  An IN-PLACE edit of a table or of ``lens_center_summary`` made since then is
        not noticed and the pass runs on the resident (older) content - call ``prepare()`` (or
        ``run``) after editing.  Another object replacing the context's tables or layout IS
        noticed (the context's tokens change) and triggers a full re-check.

        ``image``: as for ``run``; its sums stay on the GPU (``image.sums()``).  ``beam_cones``, ``beam_centre``: as for
        ``run``; the records stay in the sources' slots (``ml_farfield_beams``).  ``pupil``: as for ``run``."""
        self._check_pupil(pupil)
        beam = None
        if beam_cones is not None:
            beam_c, _back, beam_ce = _check_beam(beam_cones, beam_centre)
            beam = (beam_c, beam_ce)
        self._check_image(image)
        self.prepare(check_content=False)
        weights = np.ones(len(sources))
        for g in self._group(sources):
            self._pass(g, None, (0.0, 0.0, 0.0), weights, image, beam, pupil)

    def _group(self, sources):
        """consecutive sources at one position -> batches of up to MAX_BATCH polarisations (one
        synthesis pass with everything but two weights per sample shared); then runs of
        single-source groups at DIFFERENT positions (a field-of-view sweep) -> position batches of up
        to MAX_BATCH members (synthesised back to back before any of them is transformed).  Members
        of a group carry their own position; plane waves and dipoles do not mix."""
        groups = []
        for k, src in enumerate(sources):
            sx, sy, sz, pol = _check_source(src)
            if groups and groups[-1]['pos'] == (sx, sy, sz) and len(groups[-1]['members']) < MAX_BATCH:
                groups[-1]['members'].append((k, pol))
                groups[-1]['positions'].append((sx, sy, sz))
            else:
                groups.append({'pos': (sx, sy, sz), 'members': [(k, pol)], 'positions': [(sx, sy, sz)]})
        merged = []
        for g in groups:
            last = merged[-1] if merged else None
            single = len(g['members']) == 1
            if (single and last is not None and last.get('mixed', len(last['members']) == 1)
                    and len(last['members']) < MAX_BATCH
                    and (last['positions'][0][2] == -float('inf')) == (g['pos'][2] == -float('inf'))):
                last['members'] += g['members']
                last['positions'] += g['positions']
                last['mixed'] = True
                last['pos'] = None
            else:
                merged.append(g)
        return merged

    def _pass(self, group, slots_done, cone, weights, image=None, beam=None, pupil=None, modes=None, stokes=False, zone_fields=None):
        """queue one group: batched synthesis, then per member transform -> projection -> sums; with ``image`` the
        group's field sets are then propagated to its targets in one pass and added to the image sums; with ``beam`` =
        (cones ascending, centre or None) the beam record of each member's map is queued into the member's slot; with
        ``pupil`` the group's field sets are multiplied by it right after every synthesis, before anything reads them; with
        ``modes`` (the tables of ``_check_image_modes``) every member's image is contracted with them into the slot of its
        source right behind the image pass (``ml_propagate_modes_queue``: two launches, nothing synchronises); with ``stokes``
        the group's images are added to the image's Stokes maps as well, with the same weights; with ``zone_fields`` = (the
        ``ApertureZoneFields``, a dict) the zone contributions of the group's field sets, as they are resident at the end of the
        pass, are stored in the dict under their sources (``ml_fields_zone_fields``: this synchronises)"""
        ctx, lib = self.ctx, self.ctx.lib
        n = len(group['members'])
        params = (_lib.NearfieldParams * n)()
        for m, (k, pol) in enumerate(group['members']):
            sx, sy, sz = group['positions'][m]
            params[m] = nearfield_params(sx, sy, sz, pol, self.wavelength, self.n_glass,
                                         self.dipole_moment, self.c0, self.Z0)
        _lib.check(lib.ml_nearfield_batch_async(ctx.handle, params, n, _lib.dptr(self.x), self.x.size,
                                                _lib.dptr(self.y), self.y.size))
        if pupil is not None:
            pupil.queue(0, n)
        # member by member, each transform's second stage reading what its first stage has just
        # written (134 MB at 4096^2 -> 512^2: it is still in the 256 MB memory-side cache).  Stacking
        # the members' 4 S planes through one stage-1 launch was measured and taken out again: stage 1
        # 0.535 -> 0.512 ms for x+y+z, but stage 2 then reads a 402 MB intermediate from HBM,
        # 0.171 -> 0.268 ms (experiment log of round 4)
        for m, (k, pol) in enumerate(group['members']):
            _lib.check(lib.ml_fields_select(ctx.handle, m))
            _lib.check(lib.ml_farfield_transform_async(ctx.handle, 0, 0))
            _lib.check(lib.ml_farfield_project_async(ctx.handle, self.Z0))
            _lib.check(lib.ml_farfield_accumulate(ctx.handle, float(weights[k]), cone[0], cone[1],
                                                  cone[2], k, int(k == 0)))
            if beam is not None:
                _lib.check(lib.ml_farfield_beam(ctx.handle, 0, _lib.dptr(beam[1]), _lib.dptr(beam[0]) if beam[0].size else None,
                                                beam[0].size, k))
        if image is not None:
            # the sums start over with the group that holds source 0 (as int(k == 0) above: the first pass is
            # repeated after tie settlement and must not count twice)
            # members synthesised together at one position round a few 1e-16 differently from the source alone: their
            # field sets are written once more by the single-source kernels (the incident powers stay the batch's), so
            # that every source's image is that of the source alone
            if n > 1 and len(set(group['positions'])) == 1:
                _lib.check(lib.ml_nearfield_members_async(ctx.handle, params, n, _lib.dptr(self.x), self.x.size,
                                                          _lib.dptr(self.y), self.y.size, 1))
                if pupil is not None:
                    pupil.queue(0, n)
            image.queue_sets(0, n)
            image.accumulate([weights[k] for k, pol in group['members']], reset=group['members'][0][0] == 0)
            if stokes:
                image.accumulate_stokes([weights[k] for k, pol in group['members']], reset=group['members'][0][0] == 0)
            if modes is not None:
                if not modes['planned']:   # once per run, behind the first image pass: the image's plan is the active one now
                    image._modes_plan(modes['tx'], modes['ty'], modes['planes'], modes['n_slots'])
                    modes['planned'] = True
                for m, (k, pol) in enumerate(group['members']):
                    _lib.check(lib.ml_propagate_modes_queue(ctx.handle, m, k))
        if zone_fields is not None:
            rec = zone_fields[0].records(0, n)
            for m, (k, pol) in enumerate(group['members']):
                zone_fields[1][k] = rec[m]
        return n

    def _check_image_focus(self, image, image_radii, image_centre):
        """argument errors of ``image_radii=``, before any device call"""
        if image_radii is None:
            return
        if image is None:
            raise ValueError('image_radii= needs image=, the PlanePropagator whose sums the radii are taken in')
        if not image.want_h:
            raise ValueError('image_radii= needs an image with want_h=True: the focusing efficiency is the power sum Sz dx dy '
                             'inside a radius over the incident power')
        from .propagate import _check_focus
        _check_focus(image, image_radii, image_centre, 'sums')

    def _check_image_stokes(self, image, image_stokes, image_centre):
        """argument errors of ``image_stokes=``, before any device call -> the radii (``()`` for ``True``), or None"""
        if image_stokes is None or image_stokes is False:
            return None
        if image is None:
            raise ValueError('image_stokes= needs image=, the PlanePropagator whose images\' Stokes maps are summed')
        radii = () if image_stokes is True else image_stokes
        from .propagate import _check_focus
        _check_focus(image, radii, image_centre, 'sums', 'stokes()')
        return radii

    def _check_image_otf(self, image, image_freqs, image_centre):
        """argument errors of ``image_freqs=``, before any device call -> (fx, fy) as arrays, or None"""
        if image_freqs is None:
            return None
        if image is None:
            raise ValueError('image_freqs= needs image=, the PlanePropagator whose sums are transformed')
        try:
            fx, fy = image_freqs
        except (TypeError, ValueError):
            raise ValueError('image_freqs must be a pair (fx, fy) of frequency axes, got %r' % (image_freqs,)) from None
        from .propagate import _check_otf
        fx, fy = np.array(fx, dtype=float), np.array(fy, dtype=float)   # (taken once: the pair may be a one-shot iterable)
        _check_otf(image, fx, fy, image_centre, 'sums')
        return fx, fy

    def _check_image_modes(self, image, image_modes, n_sources):
        """argument errors of ``image_modes=``, before any device call -> the state ``_pass`` carries, or None"""
        if image_modes is None:
            return None
        if image is None:
            raise ValueError('image_modes= needs image=, the PlanePropagator whose images are contracted with the modes')
        try:
            mode_x, mode_y = image_modes
        except (TypeError, ValueError):
            raise ValueError('image_modes must be a pair (mode_x, mode_y) of mode tables, got %r' % (image_modes,)) from None
        from .propagate import _check_overlap
        tx, ty, planes, dx, dy = _check_overlap(image, mode_x, mode_y, n_slots=max(1, n_sources))
        return dict(tx=tx, ty=ty, planes=planes, dx=dx, dy=dy, n_slots=n_sources, planned=False)

    def run(self, sources, weights=None, cone=None, cone_center=(0.0, 0.0), keep_each=False, image=None,
            image_radii=None, image_centre='peak', image_freqs=None, beam_cones=None, beam_centre='peak', pupil=None,
            image_modes=None, image_stokes=None, zone_fields=None):
        """``sources`` = iterable of ``(source_x, source_y, source_z, source_pol)``; sources at the
        same position that follow each other (the x, y, z dipoles of one emitter) are synthesised
        together.  ``weights[k]`` scales source k in ``P_sum`` (default 1); ``cone`` = sine of the
        half-angle of the cone (about ``cone_center``) whose encircled power is wanted.

        Returns a dict: ``P_sum`` (incoherent sum of the far-field power maps, NaN outside the
        unit circle), ``power_in`` (incident power through the lens per source,
        nearfield.py:474-477), ``total_P`` (radiated power per source: sum of the finite
        ``P * dux * duy``, nearfield_farfield.py:74), ``efficiency`` = sum(total_P) /
        sum(power_in), ``cone_P`` / ``cone_efficiency`` if a cone was given, ``P_each`` if
        ``keep_each`` (downloads every map: for tests).

        ``image`` = a ``PlanePropagator`` built on this sweep's context and axes: the result gains ``I_sum`` =
        ``sum_k weights[k] |E_k|^2`` at its targets and, if it has ``want_h``, ``Sz_sum`` = ``sum_k weights[k]
        Sz_k`` (shape ``image.shape`` - ``(len(z), len(x), len(y))`` for a ``method='fft-stack'`` propagator, a through-focus
        volume; summed on the GPU), and with ``keep_each`` ``image_each``, the dicts of
        ``PlanePropagator.propagate()`` per source - bit for bit those of ``build_nearfield`` + ``field_at_plane`` of
        the source alone.  ``P_sum``, ``total_P``, ``power_in`` and ``cone_P`` are not touched by it (``P_each`` of
        a polarisation group is then projected from the group's re-synthesised field sets).

        ``image_radii`` = up to 32 radii in the image (needs ``image`` with ``want_h``): the result gains ``image_focus`` =
        ``image.focus(image_radii, image_centre, of='sums')`` - peak, moments and encircled sums of ``I_sum`` and ``Sz_sum``,
        reduced on the GPU (``ml_propagate_focus``) - and ``focus_efficiency`` = ``encircled_P / sum_k weights[k]
        power_in[k]``, shape ``(planes, len(image_radii))``: the power through a disc in the image plane over the incident
        power (NaN where that is 0).  ``image_centre``: ``'peak'`` (default), one ``(xc, yc)`` or ``(planes, 2)``.

        ``image_freqs`` = ``(fx, fy)``, frequency axes in cycles per length (needs ``image``): the result gains ``image_otf`` =
        ``image.otf(fx, fy, of='sums', centre=image_centre)`` - the transfer function of the field of view, the transform of
        ``I_sum`` (and ``Sz_sum``) contracted on the GPU (``ml_propagate_otf``), and its modulus, the MTF.

        ``beam_cones`` = up to 32 sines of half-angles (an empty tuple is allowed): the beam metrics of every source's far
        field, reduced on the GPU right behind its projection (``ml_farfield_beam``, one asynchronous call per source into
        the source's slot - no map is downloaded and nothing synchronises).  The result gains ``beam``, the dict of
        ``FarfieldTransform.beam`` with a leading axis over the sources - ``peak_u`` and ``centroid_u`` (where each beam
        points), ``second_moments_u`` (how wide it is), ``cone_P`` of shape ``(len(sources), len(beam_cones))``, ... -,
        ``beam_sum``, the same of ``P_sum`` (no leading axis), and ``beam_efficiency = beam['cone_P'] / power_in[:, None]``.
        ``beam_centre``: ``'peak'`` (each map's own peak direction) or one ``(ux0, uy0)``.  Takes 1 to 4095 sources (one
        slot is ``P_sum``'s).

        ``image_modes`` = ``(mode_x, mode_y)``, the tables of ``PlanePropagator.overlap`` (needs ``image``): every source's image
        is contracted with the modes on the GPU right behind its pass (``ml_propagate_modes_queue``, one asynchronous call per
        source into the source's slot; the tables are planned once, the slots are fetched at the end).  The result gains
        ``image_coupling``, the dict of ``overlap()`` with a leading axis over the sources: ``overlap_*`` of shape ``(len(sources),
        planes, nu, nv)`` - source k's have the bits of ``image.overlap()`` on that source's pass -, ``norm``, ``power`` =
        ``power_in`` per source and plane, and ``coupling_x``, ``coupling_y`` taken over each source's ``power_in``: the share of
        the emitted power that enters the mode.

        ``image_stokes`` = ``True`` or up to 32 radii in the image (needs ``image``; H is not needed): every group's images are
        added to the image's five Stokes maps beside the sums, with the same weights (``image.accumulate_stokes``).  The
        result gains ``image_stokes`` = ``image.stokes(radii, image_centre, of='sums')`` - the polarisation state of the summed
        image, its degree of polarisation for an unpolarised emitter's x, y and z dipoles - and ``image_stokes_maps`` =
        ``image.stokes_sums()``, shape ``(5,) + image.shape``.  Without it the sweep issues no call more than before.

        ``pupil`` = an ``AperturePupil`` built on this sweep's context and axes: every source's field sets are multiplied by
        it on the GPU right after their synthesis (``ml_fields_pupil_apply``, one launch per group, nothing synchronises),
        so the maps, the sums, the beam records and the image are those of the modified aperture - the cone efficiency with
        the coma removed, a ring re-phased, the outer zones stopped down.  ``power_in`` stays the incident power.

        ``zone_fields`` = an ``ApertureZoneFields`` built on this sweep's context and axes: the result gains ``zone_E``, shape
        ``(len(sources), K, 3, T)`` - every source's field at the object's points, zone by zone (``ml_fields_zone_fields`` on each
        synthesis batch's resident field sets, after the pupil if one is given; one synchronising call per batch) -, ``zone_H``
        if it has ``want_h``, and ``zone_outside_E`` / ``zone_outside_H``, shape ``(len(sources), 3, T)``."""
        self._check_pupil(pupil)
        self._check_zone_fields(zone_fields)
        beam = None
        if beam_cones is not None:
            beam_c, beam_back, beam_ce = _check_beam(beam_cones, beam_centre)
            beam = (beam_c, beam_ce)
        self._check_image(image)
        self._check_image_focus(image, image_radii, image_centre)
        image_freqs = self._check_image_otf(image, image_freqs, image_centre)
        stokes_radii = self._check_image_stokes(image, image_stokes, image_centre)
        stokes = stokes_radii is not None
        sources = list(sources)
        modes = self._check_image_modes(image, image_modes, len(sources))
        if not 1 <= len(sources) <= MAX_SLOTS:
            raise ValueError('a sweep takes 1 to %d sources, got %d' % (MAX_SLOTS, len(sources)))
        if beam is not None and len(sources) > MAX_SLOTS - 1:
            raise ValueError('a sweep with beam_cones= takes 1 to %d sources (one record slot is P_sum\'s), got %d'
                             % (MAX_SLOTS - 1, len(sources)))
        weights = np.ones(len(sources)) if weights is None else np.asarray(weights, dtype=float)
        if weights.shape != (len(sources),):
            raise ValueError('weights must have one entry per source: got shape %s for %d sources'
                             % (weights.shape, len(sources)))
        ctx, lib = self.ctx, self.ctx.lib
        self.prepare()
        cone3 = (float(cone) if cone is not None else 0.0, float(cone_center[0]), float(cone_center[1]))
        groups = self._group(sources)
        power_in = np.zeros(len(sources))
        each = [None] * len(sources)
        image_each = [None] * len(sources)
        zf = None if zone_fields is None else (zone_fields, {})
        first = True
        for g in groups:
            n = self._pass(g, None, cone3, weights, image, beam, pupil, modes, stokes, zf)
            if first:
                # exact nearest-cell ties are a property of grid and cells: settled once, by
                # asking cKDTree like the reference (ties.py), then the pass is repeated
                # (as build_nearfield does: up to three rounds - a settled tie can uncover another -
                # with the answers so far carried along; anything left after that is an error)
                ctx.sync()
                known = None
                for _ in range(3):
                    known = ties.settle(ctx, self._cells, self.x, self.y, known=known)
                    if known is None:
                        break
                    n = self._pass(g, None, cone3, weights, image, beam, pupil, modes, stokes, zf)
                    ctx.sync()
                else:
                    if ties.pending(ctx).size:
                        raise RuntimeError('nearest-cell ties still open after three rounds')
                first = False
            pw = np.zeros(n)
            _lib.check(lib.ml_nearfield_powers(ctx.handle, _lib.dptr(pw), n))
            viol = (_lib.BoundViolation * 8)()
            n_viol = _lib.c_int(0)
            _lib.check(lib.ml_nearfield_result(ctx.handle, None, viol, 8, _lib.byref(n_viol)))
            if n_viol.value:
                _raise_violation(viol[0], ctx, self.units.nm)
            for m, (k, pol) in enumerate(g['members']):
                power_in[k] = pw[m] * self.dxp * self.dyp
            if keep_each:   # the projections of this group's members, one at a time (tests)
                for m, (k, pol) in enumerate(g['members']):
                    if image is not None:
                        image_each[k] = image._download(m)
                    _lib.check(lib.ml_fields_select(ctx.handle, m))
                    _lib.check(lib.ml_farfield_transform_async(ctx.handle, 0, 0))
                    P = np.empty((self.ux.size, self.uy.size))
                    _lib.check(lib.ml_farfield_project(ctx.handle, self.Z0, _lib.dptr(P), None, None))
                    each[k] = P
        P_sum = np.empty((self.ux.size, self.uy.size))
        total_P = np.zeros(len(sources))
        cone_P = np.zeros(len(sources))
        _lib.check(lib.ml_farfield_sums(ctx.handle, _lib.dptr(P_sum), _lib.dptr(total_P),
                                        _lib.dptr(cone_P), len(sources)))
        out = {'P_sum': P_sum, 'power_in': power_in, 'total_P': total_P}
        out['efficiency'] = total_P.sum() / power_in.sum() if power_in.sum() else np.nan
        if cone is not None:
            out['cone_P'] = cone_P
            out['cone_efficiency'] = cone_P.sum() / power_in.sum() if power_in.sum() else np.nan
        if keep_each:
            out['P_each'] = each
        if beam is not None:
            S = len(sources)
            _lib.check(lib.ml_farfield_beam(ctx.handle, -1, _lib.dptr(beam_ce), _lib.dptr(beam_c) if beam_c.size else None,
                                            beam_c.size, S))
            rec = np.empty((S + 1, BEAM_RECORD))
            _lib.check(lib.ml_farfield_beams(ctx.handle, 0, S + 1, _lib.dptr(rec)))
            out['beam'] = _beam_dict(rec[:S], self.ux, self.uy, False, beam_back)
            out['beam_sum'] = _beam_single(_beam_dict(rec[S], self.ux, self.uy, False, beam_back), False)
            with np.errstate(divide='ignore', invalid='ignore'):
                out['beam_efficiency'] = np.where(power_in[:, None] != 0, out['beam']['cone_P'] / power_in[:, None], np.nan)
        if zf is not None:
            from .postprocess import _zone_fields_dict
            rec = np.stack([zf[1][k] for k in range(len(sources))])
            d = _zone_fields_dict(rec, np.zeros(rec.shape[1], dtype=np.int64), zone_fields.want_h)
            out['zone_E'], out['zone_outside_E'] = d['E'], d['outside_E']
            if zone_fields.want_h:
                out['zone_H'], out['zone_outside_H'] = d['H'], d['outside_H']
        if image is not None:
            out['I_sum'], Sz_sum = image.sums()
            if image.want_h:
                out['Sz_sum'] = Sz_sum
            if keep_each:
                out['image_each'] = image_each
            if image_radii is not None:
                out['image_focus'] = image.focus(image_radii, image_centre, of='sums')
                incident = float((weights * power_in).sum())
                enc = out['image_focus']['encircled_P']
                out['focus_efficiency'] = enc / incident if incident else np.full(enc.shape, np.nan)
            if stokes:
                out['image_stokes'] = image.stokes(stokes_radii, image_centre, of='sums')
                out['image_stokes_maps'] = image.stokes_sums()
            if image_freqs is not None:
                out['image_otf'] = image.otf(*image_freqs, of='sums', centre=image_centre)
            if modes is not None:
                from .propagate import _overlap_dict
                raw = image._modes_fetch(len(sources), modes['planes'], modes['tx'].shape[0], modes['ty'].shape[0])
                reference = np.repeat(power_in[:, None], modes['planes'], axis=1)
                out['image_coupling'] = _overlap_dict(raw, modes['tx'], modes['ty'], modes['dx'], modes['dy'], image.want_h,
                                                      image.Z0 / image._geometry[5], reference)
        return out


class WavelengthSweep:
    """Sources x WAVELENGTHS ("(source_x, source_y, source_pol, lambda) per
    launch"; the tri-colour emitter of BASELINE configs[3] on ONE GPU).

    A wavelength changes everything a context holds - the table key (nearfield.py:111), the sample
    grid (pitch lambda / 2.2, :95-97), hence the geometry records, the far-field plan - so each
    member wavelength gets a context of its own on the same GPU, and all of them stay resident
    side by side: tables, layout, records, field sets and plans are uploaded / built ONCE per
    wavelength, not once per (source, wavelength) visit as with one context re-used in turn (a
    4096^2 member is 1.2 GB of a 288 GB GPU).  The members' passes are queued on their own streams;
    nothing synchronises between them until the sums are fetched.

    ``members`` = one dict per wavelength with the arguments of ``SourceSweep`` (``wavelength``,
    ``lens_periphery_summary``, ``lens_center_summary``, ``hexgridset``, ``x_pts``, ``y_pts``,
    ``ux``, ``uy`` and optionally ``dipole_moment``, ``c0``, ``Z0``, ``units``); the lens objects may
    be shared between members (one collection list characterised at several wavelengths) or not."""

    def __init__(self, members, device=None, precision=None, method=None):
        if not members:
            raise ValueError('a wavelength sweep needs at least one member')
        self.contexts = [_lib.Context(device) for _ in members]
        self.sweeps = [SourceSweep(ctx=ctx, precision=precision, method=method, **m)
                       for ctx, m in zip(self.contexts, members)]
        self.wavelengths = [m['wavelength'] for m in members]

    def queue(self, sources):
        """queue every member's whole sweep and return without synchronising (benchmarks; see
        ``SourceSweep.queue`` for what is and is not re-checked)"""
        for sw in self.sweeps:
            sw.queue(sources)

    def sync(self):
        for ctx in self.contexts:
            ctx.sync()

    def run(self, sources, weights=None, spectrum=None, **kwargs):
        """``SourceSweep.run`` per wavelength (same sources, weights and cone).  Returns a dict:
        ``per_wavelength`` (the members' result dicts, in order) and ``efficiency`` = the spectrum-
        weighted ``sum_l s_l sum_k total_P / sum_l s_l sum_k power_in`` (``spectrum`` = relative
        spectral weights s_l, default equal); ``P_sum`` = the spectrum-weighted sum of the members'
        maps when they share one direction grid (else absent)."""
        sources = list(sources)
        s = np.ones(len(self.sweeps)) if spectrum is None else np.asarray(spectrum, dtype=float)
        if s.shape != (len(self.sweeps),):
            raise ValueError('spectrum must have one weight per wavelength')
        # (member after member: each run settles its own nearest-cell ties and reads its sums back;
        # what a member left on its context - tables, layout, records, plan - is there for the next call)
        out = [sw.run(sources, weights=weights, **kwargs) for sw in self.sweeps]
        res = {'per_wavelength': out, 'wavelengths': list(self.wavelengths)}
        num = sum(w * o['total_P'].sum() for w, o in zip(s, out))
        den = sum(w * o['power_in'].sum() for w, o in zip(s, out))
        res['efficiency'] = num / den if den else np.nan
        first = self.sweeps[0]
        if all(np.array_equal(sw.ux, first.ux) and np.array_equal(sw.uy, first.uy) for sw in self.sweeps):
            res['P_sum'] = sum(w * o['P_sum'] for w, o in zip(s, out))
        return res

    def close(self):
        for ctx in self.contexts:
            ctx.close()
