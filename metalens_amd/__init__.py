"""metalens_amd - MI355X-native near-field synthesis and near-to-far-field
transform for the sbyrnes321/metalens design flow.

Host code in Python (mirroring the reference's function and class names), compute
in hand-written HIP for gfx950 behind the C ABI of include/metalens_hip.h.
"""
from . import constants, grating, interp, layout, lens_center, postprocess, synthetic, pupil, wavefront, zones, modes  # noqa: F401
from .grating import Grating, GratingCollection  # noqa: F401
from .lens_center import HexGridSet  # noqa: F401
from .nearfield import build_nearfield, build_nearfield_big, good_fft_number  # noqa: F401
from .pipeline import HotPath  # noqa: F401
from .prepared import PreparedLens  # noqa: F401
from .sweep import SourceSweep, WavelengthSweep  # noqa: F401
from .nearfield_farfield import (FarfieldTransform, farfield_direct,  # noqa: F401
                                 farfield_from_nearfield, farfield_from_resident_nearfield,
                                 fft_direction_cosines)
from .propagate import PlanePropagator, field_at_plane  # noqa: F401
from .zones import ApertureZones, aperture_zones, zone_edges  # noqa: F401
from . import zone_fields  # noqa: F401
from .zone_fields import ApertureZoneFields, aperture_zone_fields  # noqa: F401
from .wavefront import ApertureWavefront, aperture_wavefront, zernike, zernike_terms  # noqa: F401
from .pupil import AperturePupil, apply_pupil  # noqa: F401
from .postprocess import apply_pupil_host, pupil_factor, mode_overlaps  # noqa: F401
from .postprocess import stokes_maps, stokes_metrics, analyser_power  # noqa: F401
from .modes import gaussian_axis, hermite_gauss_axis  # noqa: F401
