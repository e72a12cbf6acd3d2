from dex_ct_sim_amd.back_project import get_basismat_recon, get_recon, get_recon_covariance  # noqa: F401
