% gpu_fb_sweep_adaptive.m
% Shim for libocs.so (include/ocs.h): fb_sweep with an error control of its two passes -- the loop of the Python package's
% fb_sweep_adaptive_batch for one trajectory.  options: those of gpu_fb_sweep, and RelTol, AbsTol (default 1e-6: the
% reference's 5e-14 of fb_sweep.m:18-19 is a round-off setting for odevr7 and out of reach of RK4 meshes), InitMesh
% (default tspan), MAX_MESH_SIZE (default 20000).
% NOT VERIFIED: no MATLAB or Octave exists in the build pipeline; the same call sequence is tested through
% Python ctypes (tests/test_gpu_fb_sweep_adaptive.py).  See INTEGRATION.md.
function soln = gpu_fb_sweep_adaptive(prob, x0, tspan, options)
   if nargin < 4, options = struct(); end
   rtol = 1e-6;  atol = 1e-6;  maxNodes = 20000;  mesh = tspan(:)';
   if isfield(options, 'RelTol'), rtol = options.RelTol; end
   if isfield(options, 'AbsTol'), atol = options.AbsTol; end
   if isfield(options, 'MAX_MESH_SIZE'), maxNodes = options.MAX_MESH_SIZE; end
   if isfield(options, 'InitMesh'), mesh = options.InitMesh(:)'; end
   o = libstruct('ocs_fbs_options');  calllib('libocs', 'ocs_fbs_default_options', o);
   names = {'uRelTol', 'uAbsTol', 'nSWEEPS', 'nERROR_PTS', 'nINTERP_PTS', 'uRelax'};
   for k = 1:numel(names)
      if isfield(options, names{k}), o.(names{k}) = options.(names{k}); end
   end
   nS = numel(x0);  nC = size(prob.ControlBounds, 1);
   errorPts = linspace(mesh(1), mesh(end), o.nERROR_PTS);  interpPts = linspace(mesh(1), mesh(end), o.nINTERP_PTS);
   u0g = [];  u0e = [];  soln = struct();  meshes = [];
   while true
      integ = GpuRK4Integrator(mesh);  N = numel(mesh) - 1;  meshes(end+1) = N + 1; %#ok<AGROW>
      x = zeros(nS, N+1);  lam = x;  uI = zeros(nC, o.nINTERP_PTS);  J = 0;  sweeps = int32(0);
      [rc, ~, ~, ~, ~, ~, ~, x, lam, uI, J, sweeps] = calllib('libocs', 'ocs_fb_sweep', integ.hnd.Value, ...
            prob.h.Value, 1, x0, o, u0g, u0e, x, lam, uI, J, sweeps, []);
      if rc < 0, ocs_check(rc); end
      if sweeps == 0, status = 2; break; end                        % no converged instance on this mesh
      uFunc = vectorInterpolant(interpPts, uI, 'pchip');
      t = zeros(1, 2*N+1);  t(1:2:end) = mesh;  t(2:2:end) = (mesh(1:end-1) + mesh(2:end)) / 2;
      ugrid = uFunc(t);
      [rc, ~, ~, ~, ~, x, lam, J] = calllib('libocs', 'ocs_compute_x_lam', integ.hnd.Value, prob.h.Value, 1, x0, ugrid, x, lam, J);
      ocs_check(rc);
      rx = zeros(N, 1);  rl = rx;  rmax = rx;  rinst = 0;  errJ = 0;
      [rc, ~, ~, ~, ~, ~, ~, rx, rl, rmax, rinst, errJ] = calllib('libocs', 'ocs_x_lam_err', integ.hnd.Value, prob.h.Value, 1, ...
            ugrid, x, lam, rtol, atol, [], rx, rl, rmax, rinst, errJ);
      ocs_check(rc);
      rmax(isnan(rmax)) = inf;
      i1 = find(rmax > 1 & rmax < 32)';  i2 = find(rmax >= 32)';
      new = sort([mesh, (mesh(i1) + mesh(i1+1)) / 2, (2*mesh(i2) + mesh(i2+1)) / 3, (mesh(i2) + 2*mesh(i2+1)) / 3]);
      if numel(new) == numel(mesh), status = 0; break; end
      if numel(new) > maxNodes, status = 1; break; end
      t2 = zeros(1, 2*numel(new)-1);  t2(1:2:end) = new;  t2(2:2:end) = (new(1:end-1) + new(2:end)) / 2;
      u0g = uFunc(t2);  u0e = uFunc(errorPts);  mesh = new;
   end
   soln.mesh_status = status;  soln.meshes = meshes;  soln.mesh = mesh;
   if status ~= 2
      soln.x = vectorInterpolant(mesh, x, 'pchip');  soln.lam = vectorInterpolant(mesh, lam, 'pchip');
      soln.u = uFunc;  soln.J = J;  soln.errJ = errJ;  soln.rx = rx;  soln.rl = rl;  soln.err_ok = rinst <= 1;
   end
end
