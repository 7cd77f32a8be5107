"""Zone budget of a collimator: which Fresnel zones of the lens carry the power and which sit off phase.  The near field of
an emitter at the focus, and of one 2 um off axis, stays on the GPU and is reduced there zone by zone - the lens centre and
every grating ring - to the power through the zone, the piston of its wavefront against the collimated target wave and
how coherently the zone follows that wave; one table line per zone, nothing but 8 doubles per zone crosses PCIe (needs an
MI355X and the built library).

    python examples/zone_budget.py

The lens is the one of readme_flow.py.  The target of the off-axis emitter is the plane wave towards the direction its
chief ray takes in the glass, (ux, uy) = -(dx, dy) / sqrt(dx^2 + dy^2 + f^2) / n_glass."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(radius=100e-6, numerical_aperture=0.5, wavelength=580e-9, offset=2e-6, verbose=True):
    import metalens_amd as ma
    from metalens_amd import layout, synthetic
    lens = synthetic.make_lens((ma.Grating, ma.GratingCollection, ma.HexGridSet), layout.make_design,
                               radius=radius, numerical_aperture=numerical_aperture, wavelength=wavelength,
                               periphery_orders='physical')
    f = lens['source_distance']
    periphery, centre, hgs = lens['lens_periphery_summary'], lens['lens_center_summary'], lens['hexgridset']
    edges = ma.zone_edges(periphery)                    # zone 0: the centre, zone z: ring z - 1
    out = {'f': f, 'edges': edges}
    for name, dx in (('on_axis', 0.0), ('off_axis', offset)):
        # the reference's drop-in call; the near field stays on the GPU
        x, y, power_in, n_glass = ma.build_nearfield(dx, 0.0, -f, 'x', wavelength, periphery, centre, hgs, download=False)[4:8]
        ux = -dx / math.sqrt(dx * dx + f * f) / n_glass
        zones = ma.aperture_zones(None, None, None, None, x, y, wavelength, n_glass, edges, reference=('plane', ux, 0.0))
        out[name] = dict(zones, power_in=power_in, reference=(ux, 0.0), x=x, y=y, n_glass=n_glass)
        if not verbose:
            continue
        print('emitter %.1f um off axis: %.4g W through the lens, %.4g W leave the zones; target wave towards ux = %+.5f'
              % (dx * 1e6, power_in, zones['P'][0].sum(), ux))
        print('  zone    r_in um   r_out um  samples   P / P_in   piston rad  coherence   (x component of E)')
        inner = np.concatenate(([0.0], edges[:-1]))
        for z in range(edges.size):
            print('  %-6s %9.3f  %9.3f  %7d  %9.5f   %+9.4f   %8.4f'
                  % ('centre' if z == 0 else 'ring %d' % (z - 1), inner[z] * 1e6, edges[z] * 1e6, zones['samples'][z],
                     zones['P'][0, z] / power_in, zones['phase'][0, z, 0], zones['coherence'][0, z, 0]))
    return out


if __name__ == '__main__':
    main()
