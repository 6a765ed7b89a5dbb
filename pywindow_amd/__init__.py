"""pywindow_amd -- MI355X-native engine for pywindow's ``full_analysis()`` hot path.

The package keeps the reference's ``Molecule`` / ``MolecularSystem`` / ``DLPOLY``
API surface for that path and executes it with hand-written FP64 HIP kernels for
gfx950 (``csrc/``), through a C ABI (``include/pywindow_amd.h``) bound with
ctypes.  Nothing here falls back to a CPU: without the HIP library or a device every call raises.  (The one
CPU path that exists is explicit -- a context created with ``device=-1`` runs the same kernel source compiled for
the host, ``csrc/pw_hostpath.cpp``; nothing selects it but the caller.)
"""

import os as _os

# several kernels of one analysis run side by side on separate HIP streams; the runtime must be
# told before it initialises (harmless if the host application already set it)
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

from .distributions import (  # noqa: E402
    Distribution,
    Distribution2D,
    DistributionBand,
    block_bootstrap_counts,
    gaussian_kde_1d,
    gaussian_kde_2d,
    gaussian_kde_replicas,
)
from .correlations import TimeCorrelation, time_correlation, time_correlation_batch  # noqa: E402
from .spectra import Spectrum, dft_sums, dft_sums_batch, lomb_scargle, lomb_scargle_batch  # noqa: E402
from .gating import Gating, gate_statistics, gate_statistics_batch  # noqa: E402
from .kinetics import Kinetics, transition_counts, transition_counts_batch  # noqa: E402
from .superposition import Superposition, rmsd_matrix, superpose, superpose_batch  # noqa: E402
from .tracks import WindowTracks, track_windows  # noqa: E402
from .clustering import Clusters, cluster_frames, cluster_frames_scan  # noqa: E402
from .modes import Modes, covariance, principal_modes, project  # noqa: E402
from .cavity import Cavity, cavity_grid, cavity_grid_batch  # noqa: E402
from .surface import Surface, sphere_directions, surface_area, surface_area_batch  # noqa: E402
from .pores import PoreSizes, pore_size_distribution, pore_size_distribution_batch  # noqa: E402
from .affinity import Affinity, guest_affinity, guest_affinity_batch, lj_coefficients  # noqa: E402
from .rigid import (  # noqa: E402
    RIGID_GUESTS,
    RigidAffinity,
    RigidGuest,
    rigid_coefficients,
    rigid_guest_affinity,
    rigid_guest_affinity_batch,
)
from .rigid_body import (  # noqa: E402
    RIGID_BODIES,
    RIGID_BODY_MASSES,
    RigidBody,
    body_poses,
    rigid_body_affinity,
    rigid_body_affinity_batch,
    rotation_set,
)
from .charges import QEQ_PARAMETERS, Charges, equilibrate_charges, equilibrate_charges_batch  # noqa: E402
from .channels import Channels, channel_network, channel_network_batch  # noqa: E402
from .passage import Passage, guest_passage, guest_passage_batch, passage_field  # noqa: E402
from .percolation import Percolation, guest_percolation, guest_percolation_batch, percolation_field  # noqa: E402
from .hopping import Hopping, guest_hopping, guest_hopping_batch, window_frame  # noqa: E402
from .diffusion import Diffusion, diffusion_field, guest_diffusion, guest_diffusion_batch  # noqa: E402
from .rigid_cell import (  # noqa: E402
    RIGID_GUEST_MASSES,
    RigidField,
    rigid_guest_diffusion,
    rigid_guest_diffusion_batch,
    rigid_guest_field,
    rigid_guest_field_batch,
    rigid_guest_percolation,
    rigid_guest_percolation_batch,
)
from .ewald import EwaldPotential, ewald_parameters, ewald_potential  # noqa: E402
from .charges_cell import CellCharges, equilibrate_cell_charges, equilibrate_cell_charges_batch  # noqa: E402
from .molecular import MolecularSystem, Molecule  # noqa: E402
from .trajectory import DLPOLY  # noqa: E402
from .utilities import (  # noqa: E402
    center_of_mass,
    find_average_diameter,
    find_windows,
    max_dim,
    molecular_weight,
    opt_pore_diameter,
    pore_diameter,
    shift_com,
    sphere_volume,
)

__all__ = [
    "DLPOLY",
    "EwaldPotential",
    "ewald_parameters",
    "ewald_potential",
    "Distribution",
    "Distribution2D",
    "DistributionBand",
    "block_bootstrap_counts",
    "gaussian_kde_replicas",
    "MolecularSystem",
    "Molecule",
    "center_of_mass",
    "find_average_diameter",
    "find_windows",
    "gaussian_kde_1d",
    "gaussian_kde_2d",
    "TimeCorrelation",
    "time_correlation",
    "time_correlation_batch",
    "Spectrum",
    "dft_sums",
    "dft_sums_batch",
    "lomb_scargle",
    "lomb_scargle_batch",
    "Gating",
    "gate_statistics",
    "gate_statistics_batch",
    "Kinetics",
    "transition_counts",
    "transition_counts_batch",
    "Superposition",
    "superpose",
    "superpose_batch",
    "rmsd_matrix",
    "WindowTracks",
    "track_windows",
    "Clusters",
    "cluster_frames",
    "cluster_frames_scan",
    "Modes",
    "covariance",
    "project",
    "principal_modes",
    "Cavity",
    "cavity_grid",
    "cavity_grid_batch",
    "Surface",
    "sphere_directions",
    "surface_area",
    "surface_area_batch",
    "PoreSizes",
    "pore_size_distribution",
    "pore_size_distribution_batch",
    "Affinity",
    "guest_affinity",
    "guest_affinity_batch",
    "lj_coefficients",
    "RIGID_GUESTS",
    "RigidAffinity",
    "RigidGuest",
    "rigid_coefficients",
    "rigid_guest_affinity",
    "rigid_guest_affinity_batch",
    "RIGID_BODIES",
    "RIGID_BODY_MASSES",
    "RigidBody",
    "body_poses",
    "rotation_set",
    "rigid_body_affinity",
    "rigid_body_affinity_batch",
    "QEQ_PARAMETERS",
    "Charges",
    "equilibrate_charges",
    "equilibrate_charges_batch",
    "CellCharges",
    "equilibrate_cell_charges",
    "equilibrate_cell_charges_batch",
    "Channels",
    "channel_network",
    "channel_network_batch",
    "Passage",
    "guest_passage",
    "guest_passage_batch",
    "passage_field",
    "Percolation",
    "guest_percolation",
    "guest_percolation_batch",
    "percolation_field",
    "Diffusion",
    "guest_diffusion",
    "guest_diffusion_batch",
    "diffusion_field",
    "RIGID_GUEST_MASSES",
    "RigidField",
    "rigid_guest_field",
    "rigid_guest_field_batch",
    "rigid_guest_percolation",
    "rigid_guest_percolation_batch",
    "rigid_guest_diffusion",
    "rigid_guest_diffusion_batch",
    "Hopping",
    "guest_hopping",
    "guest_hopping_batch",
    "window_frame",
    "max_dim",
    "molecular_weight",
    "opt_pore_diameter",
    "pore_diameter",
    "shift_com",
    "sphere_volume",
]
