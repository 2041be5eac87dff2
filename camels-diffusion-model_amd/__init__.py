"""cdm_amd — MI355X-native (gfx950 HIP) ContextUnet DDPM for 64x64 CAMELS HI maps.

Drop-in for the reference's ContextUnet module API (ContextUnet.py), its diffusion helpers
(code/train_diffusion_condition.py) and the train_diffusion.py CLI.  Import as ``cdm_amd`` (the
repo-root ``cdm_amd.py`` shim maps the hyphenated directory to that name).
"""
from ._lib import lib  # noqa: F401
from .augment import augment_maps, augment_source_index, check_augment_ops, draw_augment_ops  # noqa: F401
from .diffusion import (DDPM, DDIMEncoder, DDIMSampler, DPMSolverSampler, FlowLikelihood, FlowResult,  # noqa: F401
                        GraphSampler, GuidedDDIMSampler, Program, Schedule, check_flow, check_inpaint,
                        check_observation, ddim_tables, ddim_tables_from_pairs, degrade, denoise_add_noise,
                        dpmpp_tables, dpmpp_tables_from_pairs, encode, encode_tables, flow_run_key, guided_tables,
                        known_tables, log_likelihood, perturb_input, resample_program, sample_ddpm,
                        timestep_subsequence)
from .likelihood import (FitResult, LikelihoodEvaluator, ParamFit, ParamScan, ScanResult,  # noqa: F401
                         calculate_elbo_and_bpd, calculate_elbo_and_bpd_batch, calculate_elbo_and_bpd_dataset,
                         calculate_likelihood, check_fit, check_scan, param_fit, param_grid, param_scan)
from .model import ContextUnet, EmbedFC, ResidualConvBlock, UnetDown, UnetUp  # noqa: F401
from .stats import (calculate_power_spectrum_2d, compare_distributions, compare_power_spectra,  # noqa: F401
                    pdfs, power_spectra, power_spectrum)
from .trainer import Trainer  # noqa: F401

__all__ = ["ContextUnet", "EmbedFC", "ResidualConvBlock", "UnetDown", "UnetUp", "lib", "DDPM", "GraphSampler",
           "DDIMSampler", "ddim_tables", "timestep_subsequence", "DPMSolverSampler", "dpmpp_tables",
           "known_tables", "check_inpaint", "Program", "resample_program", "ddim_tables_from_pairs",
           "dpmpp_tables_from_pairs",
           "Schedule", "denoise_add_noise", "perturb_input", "sample_ddpm", "Trainer", "LikelihoodEvaluator",
           "calculate_likelihood", "calculate_elbo_and_bpd", "calculate_elbo_and_bpd_batch",
           "calculate_elbo_and_bpd_dataset", "power_spectrum", "power_spectra", "compare_power_spectra",
           "calculate_power_spectrum_2d", "compare_distributions", "pdfs", "augment_maps", "draw_augment_ops",
           "augment_source_index", "check_augment_ops", "param_scan", "param_grid", "ParamScan", "ScanResult",
           "check_scan", "param_fit", "ParamFit", "FitResult", "check_fit", "GuidedDDIMSampler", "guided_tables",
           "check_observation", "degrade", "DDIMEncoder", "FlowLikelihood", "FlowResult", "check_flow", "encode",
           "encode_tables", "flow_run_key", "log_likelihood"]
