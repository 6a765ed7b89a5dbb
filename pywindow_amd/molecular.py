"""``Molecule`` / ``MolecularSystem`` with the reference's API surface for the hot
path (reference molecular.py:60-352, 554-836), backed by the HIP engine.

Only what ``full_analysis`` and the trajectory driver need is here: loading a
system dict, force-field key handling, ``system_to_molecule`` and the nine
``calculate_*`` methods with the reference's ``properties`` schema.  File
writers and the periodic ``rebuild_system`` are outside the accelerated path.
"""

from __future__ import annotations

from copy import deepcopy

import numpy as np

from . import _lib, engine
from .element_data import OPLS_KEY_TO_ELEMENT


class _AtomKeyError(Exception):
    def __init__(self, message: str) -> None:
        self.message = message


class _AtomKeyConflictError(Exception):
    def __init__(self, message: str) -> None:
        self.message = message


class _ForceFieldError(Exception):
    def __init__(self, message: str) -> None:
        self.message = message


def _is_number(s: str) -> bool:
    try:
        float(s)
    except ValueError:
        return False
    return True


def decipher_atom_key(atom_key: str, forcefield: str) -> str:
    """Force-field atom key -> element (reference utilities.py:267-341)."""
    ff = forcefield.upper()
    if ff in ("DLF", "DL_F"):
        head = ""
        for ch in atom_key:
            if head and _is_number(ch):
                break
            head += ch
        else:
            # the reference indexes past the end here; a key without digits is an error there too
            raise IndexError("string index out of range")
        return "".join(c for c in head if not _is_number(c) and c != "?")
    if ff in ("OPLS", "OPLSAA", "OPLS2005", "OPLS3"):
        if atom_key in ("ne", "he", "na"):
            raise _AtomKeyConflictError(
                f"One of the OPLS conflicting atom_keys has occured '{atom_key}'. "
                "For how to solve this issue see the manual or "
                "MolecularSystem._atom_key_swap() doc string."
            )
        try:
            return OPLS_KEY_TO_ELEMENT[atom_key]
        except KeyError:
            raise _AtomKeyError(
                f"OPLS atom key {atom_key} was not found in OPLS keys dictionary."
            ) from None
    raise _ForceFieldError(
        f"Unfortunetely, '{forcefield}' forcefield is not supported by pyWINDOW."
    )


class Molecule:
    """A single discrete molecule; every ``calculate_*`` runs on the GPU."""

    def __init__(self, mol: dict, system_name: str, mol_id) -> None:
        self.mol = mol
        self.no_of_atoms = len(mol["elements"])
        self.elements = mol["elements"]
        if "atom_ids" in mol:
            self.atom_ids = mol["atom_ids"]
        self.coordinates = mol["coordinates"]
        self.parent_system = system_name
        self.molecule_id = mol_id
        self.properties = {"no_of_atoms": self.no_of_atoms}
        self._cache: dict[int, np.void] = {}

    # one launch per stage set; records are cached so that chained calls
    # (pore volume -> pore diameter, ...) do not recompute -- the reference does
    # recompute (molecular.py:279, 317) but is deterministic, so results agree
    def _record(self, stages: int):
        for have, rec in self._cache.items():
            if have & stages == stages:
                return rec
        extra: list = []
        rec = engine.analyse([(self.elements, self.coordinates)], stages, extra=extra)[0]
        engine.raise_on_capacity(rec)
        self._cache = {stages: rec}
        self._more = engine.extra_by_unit(extra).get(0)      # windows beyond what a record holds
        return rec

    def _invalidate(self):
        self._cache = {}

    def full_analysis(self, ncpus: int = 1) -> dict:  # noqa: ARG002
        """All nine properties in ONE kernel launch (reference molecular.py:156-202)."""
        rec = self._record(_lib.STAGE_ALL)
        if int(rec["status"]) & _lib.ST_NEGATIVE_PORE:
            # the reference fills the dict in order and SciPy stops it at pore_diameter_opt
            # (molecular.py:196-199 -> utilities.py:422): same entries, same exception
            self.calculate_centre_of_mass()
            self.calculate_maximum_diameter()
            self.calculate_average_diameter()
            self.calculate_pore_diameter()
            self.calculate_pore_volume()
            engine.raise_like_reference(rec)
        self._fill_from(rec)
        if int(rec["status"]) & _lib.ST_TOO_FEW_POINTS:
            # molecular.py:200 -> utilities.py:1428-1431: KDTree.query(k=10) on fewer than ten sampling vectors
            del self.properties["windows"]
            raise ValueError("k must be less than or equal to the number of training points")
        return self.properties

    def _fill_from(self, rec):
        engine.warn_like_reference(rec)
        props = engine.record_to_properties(rec, more=getattr(self, "_more", None))
        self.MW = float(rec["mw"])
        self.centre_of_mass = props["centre_of_mass"]
        md = props["maximum_diameter"]
        self.maxd_atom_1, self.maxd_atom_2, self.maximum_diameter = md["atom_1"], md["atom_2"], md["diameter"]
        self.average_diameter = props["average_diameter"]
        self.pore_diameter, self.pore_closest_atom = props["pore_diameter"]["diameter"], props["pore_diameter"]["atom"]
        self.pore_volume = props["pore_volume"]
        po = props["pore_diameter_opt"]
        self.pore_diameter_opt, self.pore_opt_closest_atom, self.pore_opt_COM = (
            po["diameter"], po["atom_1"], po["centre_of_mass"])
        self.pore_volume_opt = props["pore_volume_opt"]
        # key order of the reference's dict
        for key in ("centre_of_mass", "maximum_diameter", "average_diameter", "pore_diameter",
                    "pore_volume", "pore_diameter_opt", "pore_volume_opt", "windows"):
            self.properties[key] = props[key]

    def molecular_weight(self) -> float:
        self.MW = float(self._record(_lib.STAGE_BASIC)["mw"])
        return self.MW

    def calculate_centre_of_mass(self) -> np.ndarray:
        self.centre_of_mass = np.array(self._record(_lib.STAGE_BASIC)["com"])
        self.properties["centre_of_mass"] = self.centre_of_mass
        return self.centre_of_mass

    def calculate_maximum_diameter(self) -> float:
        r = self._record(_lib.STAGE_BASIC)
        self.maxd_atom_1, self.maxd_atom_2, self.maximum_diameter = int(r["maxd_i"]), int(r["maxd_j"]), float(r["maxd"])
        self.properties["maximum_diameter"] = {
            "diameter": self.maximum_diameter, "atom_1": self.maxd_atom_1, "atom_2": self.maxd_atom_2}
        return self.maximum_diameter

    def calculate_average_diameter(self) -> float:
        self.average_diameter = float(self._record(_lib.STAGE_AVG)["avg_d"])
        self.properties["average_diameter"] = self.average_diameter
        return self.average_diameter

    def calculate_pore_diameter(self) -> float:
        r = self._record(_lib.STAGE_BASIC)
        self.pore_diameter, self.pore_closest_atom = float(r["pore_d"]), int(r["pore_atom"])
        self.properties["pore_diameter"] = {"diameter": self.pore_diameter, "atom": self.pore_closest_atom}
        return self.pore_diameter

    def calculate_pore_volume(self) -> float:
        self.calculate_pore_diameter()
        self.pore_volume = float(self._record(_lib.STAGE_BASIC)["pore_vol"])
        self.properties["pore_volume"] = self.pore_volume
        return self.pore_volume

    def calculate_pore_diameter_opt(self) -> float:
        r = self._record(_lib.STAGE_OPT)
        engine.raise_like_reference(r)
        self.pore_diameter_opt = float(r["pore_opt_d"])
        self.pore_opt_closest_atom = int(r["pore_opt_atom"])
        self.pore_opt_COM = np.array(r["pore_opt_c"])
        self.properties["pore_diameter_opt"] = {
            "diameter": self.pore_diameter_opt, "atom_1": self.pore_opt_closest_atom,
            "centre_of_mass": self.pore_opt_COM}
        return self.pore_diameter_opt

    def calculate_pore_volume_opt(self) -> float:
        self.calculate_pore_diameter_opt()
        self.pore_volume_opt = float(self._record(_lib.STAGE_OPT)["pore_vol_opt"])
        self.properties["pore_volume_opt"] = self.pore_volume_opt
        return self.pore_volume_opt

    def calculate_windows(self, ncpus: int = 1):  # noqa: ARG002
        r = self._record(_lib.STAGE_WINDOWS)
        engine.raise_like_reference(r)
        engine.warn_like_reference(r)
        if int(r["status"]) & _lib.ST_TOO_FEW_POINTS:
            raise ValueError("k must be less than or equal to the number of training points")
        win = engine.windows_of(r, getattr(self, "_more", None))
        if win is not None:
            self.properties["windows"] = {"diameters": win[0], "centre_of_mass": win[1]}
            return win[0]
        self.properties["windows"] = {"diameters": None, "centre_of_mass": None}
        return None

    def _cavity_planes(self, close):
        """The analysis that :meth:`calculate_cavity` and :meth:`calculate_pore_size_distribution` stand on -- the
        optimised pore centre, the maximum diameter and, for ``close="windows"``, the windows -- and the planes through
        the windows (``close=None``: none)."""
        from .utilities import window_planes

        if close not in ("windows", None):
            raise ValueError('close: "windows" or None')
        # (one launch for the stages this needs; the calls below read its record)
        self._record(_lib.STAGE_BASIC | _lib.STAGE_OPT | (_lib.STAGE_WINDOWS if close == "windows" else 0))
        self.calculate_pore_diameter_opt()
        self.calculate_maximum_diameter()
        if close != "windows":
            return None
        self.calculate_windows()
        return window_planes(self.pore_opt_COM, self.properties["windows"]["centre_of_mass"])

    def calculate_cavity(self, probe: float = 0.0, spacing: float = 0.5, close="windows", device=None,
                         mask: bool = False) -> float:
        """The volume of the cavity that the centre of a probe of radius ``probe`` reaches from the optimised pore
        centre (``pywindow_amd.cavity_grid``, a voxel flood fill on the GPU), closed by planes through the windows of
        ``calculate_windows`` (``close=None``: no planes) in a box of half the maximum diameter.  The reference has no
        counterpart -- its ``pore_volume_opt`` is the inscribed sphere, a lower bound.  Sets ``properties["cavity"]``:
        ``volume``, ``centre`` (the centroid), ``closed`` (``False``: the cavity reaches a face of the box, the volume
        is that of the box's part of space), ``n_voxels``, ``spacing``, ``probe``; ``self.cavity`` keeps the
        :class:`pywindow_amd.Cavity` (``mask=True``: with its voxels).  ``full_analysis`` does not call it."""
        from . import cavity as CV
        from .element_data import VDW, element_ids

        planes = self._cavity_planes(close)
        self.cavity = CV.cavity_grid(self.coordinates, VDW[element_ids(self.elements)], self.pore_opt_COM, probe, spacing,
                                     self.maximum_diameter / 2.0, planes, mask, device)
        self.properties["cavity"] = {
            "volume": float(self.cavity.volume), "centre": self.cavity.centroid, "closed": bool(self.cavity.closed),
            "n_voxels": int(self.cavity.n_voxels), "spacing": float(spacing), "probe": float(probe)}
        return self.properties["cavity"]["volume"]

    def calculate_pore_size_distribution(self, probes=None, spacing: float = 0.5, close="windows", device=None):
        """The pore sizes of the cage (``pywindow_amd.pore_size_distribution``, on the GPU): for a ladder of probe
        radii (``None``: ``0, spacing / 2, spacing, ...`` up to half the maximum diameter, at most 64) the volume a
        probe can occupy and the geometric pore size distribution, seeded at the optimised pore centre and closed by
        planes through the windows exactly as :meth:`calculate_cavity` (``close=None``: no planes), on the same grid.
        The reference has no counterpart.  Sets ``properties["pore_size_distribution"]``: ``probes``, ``diameter``,
        ``occupiable_volume``, ``histogram``, ``cumulative``, ``mean_diameter``, ``median_diameter``,
        ``largest_probe``, ``closed``, ``spacing``; ``self.pore_sizes`` keeps the :class:`pywindow_amd.PoreSizes`,
        which is returned.  ``full_analysis`` does not call it."""
        from . import pores as PS
        from .element_data import VDW, element_ids

        planes = self._cavity_planes(close)
        ps = PS.pore_size_distribution(self.coordinates, VDW[element_ids(self.elements)], self.pore_opt_COM, probes, spacing,
                                       self.maximum_diameter / 2.0, planes, False, device)
        self.pore_sizes = ps
        self.properties["pore_size_distribution"] = {
            "probes": ps.probes, "diameter": ps.diameter, "occupiable_volume": ps.occupiable_volume,
            "histogram": ps.histogram, "cumulative": ps.cumulative, "mean_diameter": float(ps.mean_diameter),
            "median_diameter": float(ps.median_diameter), "largest_probe": float(ps.largest_probe),
            "closed": bool(ps.closed), "spacing": float(spacing)}
        return ps

    def calculate_guest_affinity(self, guest="Xe", temperature: float = 298.0, spacing: float = 0.5, close="windows",
                                 device=None):
        """How strongly the cage holds a one-site Lennard-Jones guest (``pywindow_amd.guest_affinity``, on the GPU):
        the guest's energy with the UFF atoms of the cage at every voxel of the cavity of ``calculate_cavity(probe=0)``
        -- seeded, boxed and closed in the same way (``close=None``: no planes) --, a voxel within 0.5 Angstrom of an
        atom left out (``core2 = 0.25``), and the Boltzmann sums over them at ``temperature`` (K).  ``guest``: a name
        of ``pywindow_amd.affinity.GUESTS`` or a ``(sigma, eps_kJ_per_mol)`` pair.  The reference has no counterpart.
        Sets ``properties["guest_affinity"]``: ``guest``, ``temperature``, ``boltzmann_volume``, ``henry``,
        ``mean_energy``, ``heat``, ``min_energy``, ``min_position``, ``closed``, ``spacing``; ``self.affinity`` keeps
        the :class:`pywindow_amd.Affinity`, which is returned.  ``full_analysis`` does not call it."""
        from . import affinity as AF

        self.calculate_cavity(probe=0.0, spacing=spacing, close=close, device=device, mask=True)
        af = AF.guest_affinity(self.coordinates, self.elements, guest, [temperature], cavity=self.cavity, core2=0.25,
                               device=device)
        self.affinity = af
        self.properties["guest_affinity"] = {
            "guest": guest, "temperature": float(temperature), "boltzmann_volume": float(af.boltzmann_volume[0]),
            "henry": float(af.henry[0]), "mean_energy": float(af.mean_energy[0]), "heat": float(af.heat[0]),
            "min_energy": float(af.min_energy), "min_position": af.min_position, "closed": bool(af.closed),
            "spacing": float(spacing)}
        return af

    def calculate_rigid_guest_affinity(self, guest="CO2", temperature: float = 298.0, spacing: float = 0.5, close="windows",
                                       directions=None, charges=None, device=None, rotations=None):
        """How strongly the cage holds a rigid linear guest -- N2, CO2, O2 -- averaged over its orientations
        (``pywindow_amd.rigid_guest_affinity``, on the GPU): the guest's centre at every voxel of the cavity of
        ``calculate_cavity(probe=0)`` -- seeded, boxed and closed as in :meth:`calculate_guest_affinity` --, in every
        one of ``directions`` (``None``: ``pywindow_amd.sphere_directions`` of ``pywindow_amd.rigid.M_DEFAULT``), a
        pose with a site within 0.5 Angstrom of an atom left out (``core2 = 0.25``).  ``guest``: a name of
        ``pywindow_amd.rigid.RIGID_GUESTS`` or a :class:`pywindow_amd.RigidGuest`.  ``charges``: the framework's
        partial charges in e, one per atom, or ``"qeq"``: the library's own (:meth:`calculate_charges`); ``None``: no
        electrostatics at all (the bundled cage model carries no charges, and the guest's then do nothing).  The reference has no counterpart.  Sets
        ``properties["rigid_guest_affinity"]``: ``guest``, ``temperature``, ``boltzmann_volume``, ``henry``,
        ``mean_energy``, ``heat``, ``min_energy``, ``min_position``, ``min_direction``, ``closed``, ``spacing``;
        ``self.rigid_affinity`` keeps the :class:`pywindow_amd.RigidAffinity`, which is returned.  ``full_analysis``
        does not call it.  A rigid body -- a name of ``pywindow_amd.RIGID_BODIES`` (H2O, CH4, SF6) or a
        :class:`pywindow_amd.RigidBody` -- goes through ``pywindow_amd.rigid_body_affinity`` instead, averaged over
        ``rotations`` (``None``: ``pywindow_amd.rotation_set()``); the properties then also hold ``min_rotation``."""
        from . import rigid as RG
        from . import rigid_body as RB

        body = RB.is_body(guest)
        if (directions is not None and body) or (rotations is not None and not body):
            raise ValueError("calculate_rigid_guest_affinity: directions for a linear guest, rotations for a rigid body")
        self.calculate_cavity(probe=0.0, spacing=spacing, close=close, device=device, mask=True)
        if body:
            af = RB.rigid_body_affinity(self.coordinates, self.elements, guest, [temperature], cavity=self.cavity,
                                        rotations=rotations, charges=charges, core2=0.25, device=device)
        else:
            af = RG.rigid_guest_affinity(self.coordinates, self.elements, guest, [temperature], cavity=self.cavity,
                                         directions=directions, charges=charges, core2=0.25, device=device)
        self.rigid_affinity = af
        self.properties["rigid_guest_affinity"] = {
            "guest": guest, "temperature": float(temperature), "boltzmann_volume": float(af.boltzmann_volume[0]),
            "henry": float(af.henry[0]), "mean_energy": float(af.mean_energy[0]), "heat": float(af.heat[0]),
            "min_energy": float(af.min_energy), "min_position": af.min_position, "min_direction": af.min_direction,
            "closed": bool(af.closed), "spacing": float(spacing)}
        if body:
            self.properties["rigid_guest_affinity"]["min_rotation"] = af.min_rotation
        return af

    def calculate_charges(self, total_charge: float = 0.0, device=None):
        """The partial charges of the molecule by charge equilibration (``pywindow_amd.equilibrate_charges``, on the
        GPU; ``QEQ_PARAMETERS`` of :mod:`pywindow_amd.charges`, which also says what the model leaves out).  The
        reference has no counterpart.  Sets ``properties["charges"]`` and ``self.charges`` to the ``(n,)`` charges in e
        and ``self.charge_equilibration`` to the :class:`pywindow_amd.Charges`; returns the charges.  They are what
        ``calculate_rigid_guest_affinity(charges="qeq")`` uses.  ``full_analysis`` does not call it."""
        from . import charges as CH

        result = CH.equilibrate_charges(self.coordinates, self.elements, total_charge, device=device)
        self.charge_equilibration = result
        self.charges = result.charges
        self.properties["charges"] = result.charges
        return result.charges

    def calculate_guest_passage(self, guest="Xe", spacing: float = 0.5, close="windows", device=None):
        """What it costs a one-site Lennard-Jones guest to leave the cage through each window
        (``pywindow_amd.guest_passage``, on the GPU): the guest's energy with the UFF atoms of the cage at every voxel
        of the box of ``calculate_cavity`` -- the same grid, seed and planes through the windows --, and per window,
        with the other windows' planes shut, the lowest energy level that connects the pore centre to the outside
        (``barrier``), the lowest energy inside it (``well``) and their difference, the activation energy of the hop for
        the cage as it stands.  ``close=None``: one row without planes, the cheapest way out of the box.  ``guest``: a
        name of ``pywindow_amd.affinity.GUESTS`` or a ``(sigma, eps_kJ_per_mol)`` pair.  The reference has no
        counterpart.  Sets ``properties["guest_passage"]``: ``guest``, ``barrier``, ``well``, ``activation``,
        ``saddle_position``, ``free_exit``, ``no_exit``, ``n_windows``, ``spacing``; ``self.passage`` keeps the
        :class:`pywindow_amd.Passage`, which is returned.  ``full_analysis`` does not call it."""
        from . import passage as PA

        planes = self._cavity_planes(close)
        ps = PA.guest_passage(self.coordinates, self.elements, guest, self.pore_opt_COM, planes, spacing,
                              self.maximum_diameter / 2.0, core2=0.25, device=device)
        self.passage = ps
        self.properties["guest_passage"] = {
            "guest": guest, "barrier": ps.barrier.copy(), "well": ps.well.copy(), "activation": ps.activation,
            "saddle_position": ps.saddle_position, "free_exit": ps.free_exit, "no_exit": ps.no_exit,
            "n_windows": int(ps.n_windows), "spacing": float(spacing)}
        return ps

    def calculate_guest_hopping(self, guest="Xe", temperature: float = 298.0, spacing: float = 0.25, device=None):
        """How fast a one-site Lennard-Jones guest hops out of the cage through each window
        (``pywindow_amd.guest_hopping``, on the GPU): the free-energy profile of the guest along the line from the
        optimised pore centre through every window of ``calculate_windows``, the other windows' planes shut, and the
        transition-state-theory rate ``sqrt(k_B T / 2 pi m) * area / well_volume`` at ``temperature`` (K) for the cage
        as it stands.  ``guest``: a name of ``pywindow_amd.affinity.GUESTS``.  The reference has no counterpart.  Sets
        ``properties["guest_hopping"]``: ``guest``, ``temperature``, ``rate``, ``free_barrier``, ``area``,
        ``well_volume``, ``escape_rate``, ``valid``, ``free_exit``, ``n_windows``, ``spacing``; ``self.hopping`` keeps
        the :class:`pywindow_amd.Hopping`, which is returned.  ``full_analysis`` does not call it."""
        from . import hopping as HP

        self._cavity_planes("windows")
        hp = HP.guest_hopping(self.coordinates, self.elements, guest, self.pore_opt_COM,
                              self.properties["windows"]["centre_of_mass"], [temperature], spacing, device=device)
        self.hopping = hp
        self.properties["guest_hopping"] = {
            "guest": guest, "temperature": float(temperature), "rate": hp.rate[:, 0].copy(),
            "free_barrier": hp.free_barrier[:, 0].copy(), "area": hp.area[:, 0].copy(),
            "well_volume": hp.well_volume[:, 0].copy(), "escape_rate": float(hp.escape_rate[0]),
            "valid": hp.valid[:, 0].copy(), "free_exit": hp.free_exit[:, 0].copy(), "n_windows": int(hp.n_windows[0]),
            "spacing": float(spacing)}
        return hp

    def calculate_surface_area(self, probe: float = 0.0, points: int = 960, side=None, device=None) -> float:
        """The solvent-accessible surface area for a probe of radius ``probe`` (``pywindow_amd.surface_area``, Shrake
        and Rupley's test points on the GPU, ``points`` an atom).  ``side=None``: the whole surface, no analysis is
        run.  ``side="internal"`` / ``"external"``: the part that faces the cavity / the outside -- the analysis and
        ``calculate_cavity(probe)`` run first, with the same planes through the windows, and the cavity's voxels say
        which side an exposed point is on.  The reference has no counterpart.  Sets ``properties["surface_area"]``:
        ``area``, ``internal_area`` and ``external_area`` (``None`` without a side), ``closed`` (the cavity's),
        ``probe``, ``points``; ``self.surface`` keeps the :class:`pywindow_amd.Surface`.  ``full_analysis`` does not
        call it."""
        from . import surface as SF
        from .element_data import VDW, element_ids

        if side not in (None, "internal", "external"):
            raise ValueError('side: None, "internal" or "external"')
        cav = None
        if side is not None:
            self.calculate_cavity(probe=probe, device=device, mask=True)
            cav = self.cavity
        self.surface = SF.surface_area(self.coordinates, VDW[element_ids(self.elements)], probe, points, cav, device)
        sided = side is not None
        self.properties["surface_area"] = {
            "area": float(self.surface.area),
            "internal_area": float(self.surface.internal_area) if sided else None,
            "external_area": float(self.surface.external_area) if sided else None,
            "closed": bool(self.surface.closed) if sided else None, "probe": float(probe), "points": int(points)}
        return self.properties["surface_area"][{None: "area", "internal": "internal_area", "external": "external_area"}[side]]

    def _align_to_principal_axes(self, align_molsys: bool = False) -> None:
        """Reference molecular.py:204-213.  There the result -- a ``(coordinates, rotations)`` tuple -- is
        assigned to ``self.coordinates[0]``, which numpy refuses; here the molecule takes the aligned
        coordinates (what the method's name promises) and keeps the rotations."""
        if align_molsys:
            raise NotImplementedError
        from .utilities import align_principal_ax

        aligned, self.principal_axes_rotations = align_principal_ax(self.elements, self.coordinates)
        self.coordinates = aligned
        self.mol["coordinates"] = aligned
        self.aligned_to_principal_axes = True
        self._invalidate()

    def shift_to_origin(self) -> None:
        com = self.calculate_centre_of_mass()
        self.coordinates = np.asarray(self.coordinates, float) - np.array([com] * self.no_of_atoms)
        self.mol["coordinates"] = self.coordinates
        self._invalidate()


class MolecularSystem:
    """Container of a (possibly multi-molecule) system (reference molecular.py:554-836)."""

    def __init__(self) -> None:
        self.system_id = 0
        self.system: dict = {}

    @classmethod
    def load_system(cls, dict_: dict, system_id: str | int = "system") -> "MolecularSystem":
        obj = cls()
        obj.system = dict_
        obj.system_id = system_id
        return obj

    @classmethod
    def load_file(cls, filepath) -> "MolecularSystem":
        """Load an ``.xyz`` or ``.pdb`` file (reference molecular.py:596-623 with the readers of
        io_tools.py:106-182; CRYST1 becomes ``unit_cell`` and ``lattice``)."""
        import pathlib

        from .rebuild import unit_cell_to_lattice_array

        path = pathlib.Path(filepath)
        lines = path.read_text().splitlines(keepends=True)
        system: dict = {}
        if path.suffix == ".xyz":
            body = [ln.split() for ln in lines[2:]]
            try:
                system["elements"] = np.array([b[0] for b in body])
                system["coordinates"] = np.array([[float(b[1]), float(b[2]), float(b[3])] for b in body])
            except IndexError:
                raise ValueError("The XYZ file is corrupted in some way (empty line at the end, or a trajectory).") from None
        elif path.suffix == ".pdb":
            if sum(ln.count("END ") for ln in lines) > 1:
                raise ValueError("Multiple 'END' statements were found in this PDB file.")
            atoms = [ln for ln in lines if ln[:6] in ("HETATM", "ATOM  ")]
            system["remarks"] = [ln for ln in lines if ln[:6] == "REMARK"]
            system["unit_cell"] = np.array([
                float(x) for ln in lines if ln[:6] == "CRYST1"
                for x in (ln[6:15], ln[15:24], ln[24:33], ln[33:40], ln[40:47], ln[47:54])
            ])
            if system["unit_cell"].any():
                system["lattice"] = unit_cell_to_lattice_array(system["unit_cell"])
            system["atom_ids"] = np.array([ln[12:16].strip() for ln in atoms], dtype="<U8")
            system["elements"] = np.array([ln[76:78].strip() for ln in atoms], dtype="<U8")
            system["coordinates"] = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in atoms])
        else:
            raise ValueError(f"unsupported file type {path.suffix!r} (xyz and pdb are read natively)")
        obj = cls()
        obj.system = system
        obj.filename = path.name
        obj.system_id = path.name.split(".")[0]
        return obj

    def rebuild_system(self, override: bool = False) -> "MolecularSystem":
        """Re-assemble the molecules of a periodic system through the cell faces
        (reference molecular.py:672-708); the 3x3x3 supercell and the bonded-neighbour walk
        run on the GPU (csrc/pw_rebuild.hpp)."""
        from .rebuild import discrete_molecules

        discrete = discrete_molecules(self.system, rebuild=True)
        coordinates = np.array([], dtype=np.float64).reshape(0, 3)
        atom_ids = np.array([])
        elements = np.array([])
        for mol in discrete:
            coordinates = np.concatenate([coordinates, mol["coordinates"]], axis=0)
            atom_ids = np.concatenate([atom_ids, mol["atom_ids"]], axis=0)
            elements = np.concatenate([elements, mol["elements"]], axis=0)
        rebuilt = {"coordinates": coordinates, "atom_ids": atom_ids, "elements": elements}
        if override is True:
            self.system.update(rebuilt)
        return self.load_system(rebuilt)

    def make_modular(self, rebuild: bool = False) -> None:
        """Populate ``self.molecules`` with the discrete molecules of the system
        (reference molecular.py:798-824)."""
        from .rebuild import discrete_molecules

        dis = discrete_molecules(self.system, rebuild=True if rebuild is True else None)
        self.no_of_discrete_molecules = len(dis)
        self.molecules = {}
        for i in range(len(dis)):
            self.molecules[i] = Molecule(dis[i], str(self.system_id), i)

    def calculate_channels(self, probe=0.0, spacing: float = 0.5, c_max: int = 64, mask: bool = False, labels: bool = False,
                           device=None):
        """The pore network of the loaded cell (``pywindow_amd.channel_network``, ``pw_channels`` on the GPU): the
        periodic components of its void for a probe of radius ``probe`` (a sequence: a ladder of probes), their ranks
        -- pocket, channel, layer, network -- and the accessible and inaccessible volume, with the van der Waals radii
        of ``element_data.VDW``.  Needs ``elements`` and a ``lattice`` or ``unit_cell``; the result, a
        :class:`pywindow_amd.Channels`, is also kept in ``self.channels``."""
        from . import channels as CN
        from .rebuild import system_lattice

        if "elements" not in self.system:
            raise KeyError("elements")
        lattice, periodic = system_lattice(self.system)
        if not periodic:
            raise ValueError("calculate_channels: the system has no unit cell (a 'lattice' or a 'unit_cell' is needed)")
        self.channels = CN.channel_network(self.system["coordinates"], self.system["elements"], lattice, probe, spacing,
                                           c_max, mask, labels, device)
        return self.channels

    def calculate_guest_percolation(self, guest="Xe", spacing: float = 0.5, cutoff: float = 12.0, core2: float = 0.25,
                                    maps: bool = False, device=None):
        """The energy levels at which the voids of the loaded cell connect for a one-site Lennard-Jones guest
        (``pywindow_amd.guest_percolation``, ``pw_percolation`` on the GPU, UFF atoms): the minimax barrier of
        diffusion in at least 1, 2, 3 dimensions and along each cell vector, with the well below it.  Needs ``elements``
        and a ``lattice`` or ``unit_cell``; the result, a :class:`pywindow_amd.Percolation`, is also kept in
        ``self.percolation``."""
        from . import percolation as PC
        from .rebuild import system_lattice

        if "elements" not in self.system:
            raise KeyError("elements")
        lattice, periodic = system_lattice(self.system)
        if not periodic:
            raise ValueError("calculate_guest_percolation: the system has no unit cell (a 'lattice' or a 'unit_cell' is needed)")
        self.percolation = PC.guest_percolation(self.system["coordinates"], self.system["elements"], lattice, guest, spacing,
                                                cutoff, core2, maps, device)
        return self.percolation

    def calculate_guest_diffusion(self, guest="Xe", temperatures=298.0, spacing: float = 0.5, cutoff: float = 12.0,
                                  core2: float = 0.25, cap: float = 100.0, merge=None, mass=None, maps: bool = False,
                                  labels: bool = False, device=None):
        """The self-diffusion tensor of a one-site Lennard-Jones guest through the loaded cell
        (``pywindow_amd.guest_diffusion``, ``pw_basins`` on the GPU, UFF atoms): the hop network between the energy basins
        of the guest's landscape and its tensor at every temperature.  Needs ``elements`` and a ``lattice`` or
        ``unit_cell``; the result, a :class:`pywindow_amd.Diffusion`, is also kept in ``self.diffusion``."""
        from . import diffusion as DF
        from .rebuild import system_lattice

        if "elements" not in self.system:
            raise KeyError("elements")
        lattice, periodic = system_lattice(self.system)
        if not periodic:
            raise ValueError("calculate_guest_diffusion: the system has no unit cell (a 'lattice' or a 'unit_cell' is needed)")
        self.diffusion = DF.guest_diffusion(self.system["coordinates"], self.system["elements"], lattice, guest, temperatures,
                                            spacing, cutoff, core2, cap, merge, mass, maps, labels, device)
        return self.diffusion

    def _rigid_cell_inputs(self, what):
        from .rebuild import system_lattice

        if "elements" not in self.system:
            raise KeyError("elements")
        lattice, periodic = system_lattice(self.system)
        if not periodic:
            raise ValueError(f"{what}: the system has no unit cell (a 'lattice' or a 'unit_cell' is needed)")
        return self.system["coordinates"], self.system["elements"], lattice

    def calculate_cell_charges(self, cutoff: float = 12.0, tolerance: float = 1e-6, shield=(4.0, 6.0), tol: float = 1e-10,
                               max_iter: int = 1000, device=None):
        """The partial charges of every atom of the loaded cell by periodic charge equilibration
        (``pywindow_amd.equilibrate_cell_charges``, ``pw_charges_cell`` on the GPU; ``QEQ_PARAMETERS`` of
        :mod:`pywindow_amd.charges`; :mod:`pywindow_amd.charges_cell` says what the model leaves out and why ``shield`` is a
        model parameter).  Needs ``elements`` and a ``lattice`` or ``unit_cell``.  The result, a
        :class:`pywindow_amd.CellCharges`, is also kept in ``self.cell_charges``; it is what
        ``calculate_rigid_guest_percolation(charges="qeq-cell")`` and ``_diffusion`` make for themselves."""
        from . import charges_cell as CC

        xyz, elements, lattice = self._rigid_cell_inputs("calculate_cell_charges")
        self.cell_charges = CC.equilibrate_cell_charges(xyz, elements, lattice, cutoff, tolerance, shield, tol, max_iter, device)
        return self.cell_charges

    def calculate_rigid_guest_percolation(self, guest="CO2", temperatures=298.0, spacing: float = 0.5, cutoff: float = 12.0,
                                          core2: float = 0.25, directions=None, device=None, charges=None,
                                          ewald_tolerance: float = 1e-6):
        """The levels at which the free-energy landscape of a rigid linear guest's centre (N2, CO2, O2 or a
        :class:`pywindow_amd.RigidGuest`) connects through the loaded cell (``pywindow_amd.rigid_guest_percolation``:
        ``pw_rigid_cell``, then ``pw_percolation`` on the GPU, UFF atoms): a list, one
        :class:`pywindow_amd.Percolation` per temperature, also kept in ``self.rigid_percolation``.  ``charges`` (the framework's point charges in e, one per atom or one row a frame) and
        ``ewald_tolerance``: the Ewald sum of ``pywindow_amd.rigid_guest_field``; ``"qeq-cell"``: the charges of
        :meth:`calculate_cell_charges` at the same cutoff and tolerance; ``None``: uncharged, ``pw_rigid_cell``."""
        from . import rigid_cell as RC

        xyz, elements, lattice = self._rigid_cell_inputs("calculate_rigid_guest_percolation")
        self.rigid_percolation = RC.rigid_guest_percolation(xyz, elements, lattice, guest, temperatures, spacing, cutoff, core2,
                                                            directions, device, charges=charges, ewald_tolerance=ewald_tolerance)
        return self.rigid_percolation

    def calculate_rigid_guest_diffusion(self, guest="CO2", temperatures=298.0, spacing: float = 0.5, cutoff: float = 12.0,
                                        core2: float = 0.25, directions=None, cap: float = 100.0, merge=None, mass=None,
                                        labels: bool = False, device=None, charges=None, ewald_tolerance: float = 1e-6):
        """The self-diffusion tensor of a rigid linear guest through the loaded cell
        (``pywindow_amd.rigid_guest_diffusion``: ``pw_rigid_cell``, then ``pw_basins`` on the GPU, UFF atoms), each
        temperature on its own free-energy field: a :class:`pywindow_amd.Diffusion`, also kept in
        ``self.rigid_diffusion``.  ``charges`` (the framework's point charges in e, one per atom or one row a frame) and
        ``ewald_tolerance``: the Ewald sum of ``pywindow_amd.rigid_guest_field``; ``"qeq-cell"``: the charges of
        :meth:`calculate_cell_charges` at the same cutoff and tolerance; ``None``: uncharged, ``pw_rigid_cell``."""
        from . import rigid_cell as RC

        xyz, elements, lattice = self._rigid_cell_inputs("calculate_rigid_guest_diffusion")
        self.rigid_diffusion = RC.rigid_guest_diffusion(xyz, elements, lattice, guest, temperatures, spacing, cutoff, core2,
                                                        directions, cap, merge, mass, labels, device, charges=charges,
                                                        ewald_tolerance=ewald_tolerance)
        return self.rigid_diffusion

    def swap_atom_keys(self, swap_dict: dict, dict_key: str = "atom_ids") -> None:
        """Reference molecular.py:710-749."""
        if "atom_ids" not in self.system:
            dict_key = "elements"
        for atom_key in range(len(self.system[dict_key])):
            for key in swap_dict:
                if self.system[dict_key][atom_key] == key:
                    self.system[dict_key][atom_key] = swap_dict[key]

    def decipher_atom_keys(self, forcefield: str = "DLF", dict_key: str = "atom_ids") -> None:
        """Reference molecular.py:751-796."""
        if "atom_ids" not in self.system:
            dict_key = "elements"
        temp = deepcopy(self.system[dict_key])
        for element in range(len(temp)):
            temp[element] = str(decipher_atom_key(temp[element], forcefield=forcefield))
        self.system["elements"] = temp

    def system_to_molecule(self) -> Molecule:
        return Molecule(self.system, self.system_id, 0)
