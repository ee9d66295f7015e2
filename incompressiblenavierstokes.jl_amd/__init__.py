"""MI355X-native hot path of IncompressibleNavierStokes.jl behind the reference's own API names.

Julia's `op!` is spelled `op_` here; indices are 0-based; `backend = ...` becomes `device = ...`.
Everything numerical runs in hand-written HIP kernels + rocFFT inside libinship.so (C ABI:
include/ins_hip.h).  There is no CPU fallback: importing this package without the built library, or
creating a `Setup` without a HIP device, raises.
"""
from . import _lib
from . import f32  # noqa: F401  (the `_f32` entry-point family, T = Float32)
from ._lib import INSHipError
from .boundary_conditions import DirichletBC, HaloBC, PeriodicBC, PressureBC, SymmetricBC
from .distributed import AbiSlabComm, HipSlabKernels, SlabComm, SlabLayout, SlabStepper
from .grid import Grid, cosine_grid, max_size, stretched_grid, tanh_grid
from .initializers import random_field, temperaturefield, velocityfield
from .operators import (
    Dfield,
    Dfield_,
    Qfield,
    Qfield_,
    apply_bc_p,
    apply_bc_p_,
    apply_bc_p_pullback_,
    apply_bc_u_pullback_,
    convection_adjoint_,
    diffusion_adjoint_,
    divergence_adjoint_,
    momentum_pullback_,
    pressuregradient_adjoint_,
    apply_bc_temp,
    apply_bc_temp_,
    apply_bc_temp_pullback_,
    convection_diffusion_temp_adjoint_,
    dissipation_adjoint_,
    gravity_adjoint_,
    temperature_pullback_,
    applybodyforce,
    applybodyforce_,
    convection_diffusion_temp,
    convection_diffusion_temp_,
    dissipation,
    dissipation_,
    dissipation_from_strain,
    dissipation_from_strain_,
    divoftensor_,
    divoftensor_adjoint_,
    eig2field,
    eig2field_,
    gravity,
    gravity_,
    interpolate_u_p,
    interpolate_u_p_,
    interpolate_ω_p,
    interpolate_ω_p_,
    smagorinsky_closure,
    smagtensor_,
    tensorbasis,
    tensorbasis_,
    tensorbasis_matrices,
    tensorbasis_pullback_,
    tensorclosure_pullback_,
    tensorclosure_stress_,
    tensorinvariants_,
    tensorfield,
    vorticity,
    vorticity_,
    apply_bc_u,
    apply_bc_u_,
    applypressure,
    applypressure_,
    convection,
    convection_,
    convectiondiffusion_,
    diffusion,
    diffusion_,
    divergence,
    divergence_,
    kinetic_energy,
    kinetic_energy_,
    laplacian,
    laplacian_,
    max_abs_divergence,
    momentum,
    momentum_,
    pressuregradient,
    pressuregradient_,
    scalewithvolume,
    scalewithvolume_,
    total_kinetic_energy,
)
from .pressure import (
    default_psolver,
    poisson,
    poisson_,
    pressure,
    project,
    project_,
    project_pullback_,
    psolver_cg,
    psolver_direct,
    psolver_spectral,
)
from .processors import (Observable, fieldsaver, get_scale_numbers, observefield, observespectrum, observespectrum_ensemble, processor, save_vtk, spectral_stuff, timelogger,
                         vtk_writer)
from .setup import Setup, copyfield, from_numpy, scalarfield, temperature_equation, to_numpy, vectorfield, vectorfields
from .sciml import create_right_hand_side, right_hand_side_
from .solver import get_cfl_timestep_, get_state, solve_unsteady, solve_unsteady_ensemble
from .time_steppers import (
    EnsembleCache,
    ExplicitRungeKuttaMethod,
    LMWray3,
    RKMethods,
    create_stepper,
    ensemble_apply_bc_u_,
    ensemble_apply_bc_u_pullback_,
    ensemble_momentum_,
    ensemble_momentum_pullback_,
    ensemble_project_,
    ensemble_project_pullback_,
    ensemble_rhs_,
    ensemble_stats,
    get_cfl_timestep_ensemble,
    ode_method_cache,
    runge_kutta_method,
    timestep,
    timestep_,
    timesteps_,
    timesteps_ensemble_,
)
from . import autodiff as ad  # noqa: E402  (torch.autograd Functions over the pullback kernels: ins_amd.ad)
from . import autodiff32 as ad32  # noqa: E402  (the same over float32 fields and the `_f32` pullbacks: ins_amd.ad32)

from . import neuralclosure  # noqa: E402  (lib/NeuralClosure: filters, filtered-DNS data generation, closures, losses, training)
from .neuralclosure import (FaceAverage, VolumeAverage, cnn, collocate, create_dataloader_post, create_dataloader_prior,  # noqa: E402
                            create_io_arrays, create_les_data, create_les_data_ensemble, create_loss_post, create_loss_post_ensemble, create_loss_prior, create_relerr_post, create_relerr_prior,
                            decollocate, filtersaver, lesdatagen, reconstruct, reconstruct_, tensorclosure, train, wrappedclosure, wrappedclosure_ensemble)

_lib.load()  # fail loudly at import time if libinship.so is absent
